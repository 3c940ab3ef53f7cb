"""The spectrogram stage's kernels (aad_amd/csrc/aad_spectrogram.hip, namespace aad::spectrum), one record per instantiation, and
the inputs of the cases of tests/test_gpu_spectrogram.py, which tests/test_spectrogram_host.py runs its numpy mutants on.
tests/test_spectrogram_kernel_census.py holds the built library to exactly the records.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import os
import re
import subprocess
from collections import namedtuple

import numpy as np

from kernel_names import ARG

import spectrogram_oracle as so

GPU_FILE = "test_gpu_spectrogram.py"
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "aad_amd", "csrc")

Cell = namedtuple("Cell", "kernel args case")

# _ZN3aad8spectrum <length> <name> I <arguments> E E: kernel_names.NAME with the nested namespace in front; that pattern and
# convolve_matrix.NAME read "8spectrum..." as no name of theirs
NAME = re.compile(rb"_ZN3aad8spectrum(\d+)([a-z][a-z0-9_]*_kernel)(?:I((?:L[ib]n?\d+E)+)E)?E")


def kernels_in(data):
    """bytes -> the set of (kernel, template arguments) among the mangled names of aad::spectrum kernels in them"""
    found = set()
    for m in NAME.finditer(data):
        name = m.group(2)
        if int(m.group(1)) != len(name):
            continue
        found.add((name.decode(), tuple(-int(v) if neg else int(v) for _, neg, v in ARG.findall(m.group(3) or b""))))
    return found


def cells():
    """MEL false: the power spectrum from the lanes; MEL true: the filterbank behind the hand-off buffer"""
    return [Cell("spectrum_rows_kernel", (0,), "test_small_every_edge"), Cell("spectrum_rows_kernel", (1,), "test_small_every_edge")]


# ---- the header through g++ ----------------------------------------------------------------------------------------------------------

def build_driver(directory):
    exe = os.path.join(str(directory), "spectrogram_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", exe, os.path.join(HERE, "spectrogram_driver.cpp")],
                   check=True)
    return exe


def ask(driver, *words):
    return subprocess.run([driver] + [str(w) for w in words], check=True, capture_output=True, text=True).stdout.splitlines()


def geometry(driver, W, H):
    """-> (pitch, tile_frames, frame_major, plane_elements, lds bytes with filters) of aad::spectrum_geometry"""
    return tuple(int(v) for v in ask(driver, "geometry", W, H)[0].split())


# ---- the small case: every edge ------------------------------------------------------------------------------------------------------

SMALL_FFT, SMALL_W = 96, 80  # B = 49: two k-steps, the second with 16 taps; four column tile pairs, the last with one bin
SMALL_HOPS = (16, 37, 80, 96)
ROW_NAMES = ("noise", "minus_rail", "alternating_rails", "silence")


def small_frames(H, tile_frames):
    """T for which F is one more than the frame tile"""
    return SMALL_W + tile_frames * H


def hand_made_rows(T, seed=5):
    rng = np.random.default_rng(seed)
    rows = np.zeros((4, T), dtype=np.int16)
    rows[0] = rng.integers(-32768, 32768, size=T)
    rows[1] = -32768
    rows[2] = np.where(np.arange(T) % 2 == 0, 32767, -32768)
    return rows


def awkward_filters(B):
    """an all-zero filter, one with a zero inside its band, one with a negative weight, one that covers every bin, and one on
    the last two bins - across the last column tile's edge when B = 16 n + 1"""
    rng = np.random.default_rng(11)
    f = np.zeros((5, B), dtype=np.float32)
    f[1, 3:10] = [0.25, 0.5, 0.75, 0.0, 0.75, 0.5, 0.25]
    f[2, 13:20] = [0.3, 0.6, -0.75, 1.0, 0.7, 0.4, 0.1]
    f[3] = rng.uniform(0.1, 1.0, size=B)
    f[4, B - 2:] = [0.5, 1.5]
    return f


def strided(rows, extra, parity):
    """the rows `extra` elements further apart with rails behind every row's end, the first at element `parity` of the buffer
    -> (buffer int16, offset, pitch)"""
    R, T = rows.shape
    pitch = T + extra
    buf = np.where(np.arange(parity + R * pitch) % 3 == 0, 32767, -32768).astype(np.int16)
    for r in range(R):
        buf[parity + r * pitch: parity + r * pitch + T] = rows[r]
    return buf, parity, pitch


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------

Shape = namedtuple("Shape", "n_fft W H T rows mels")
SHAPES = {
    "one_step": Shape(128, 64, 48, 64 + 48 * 20, 2, 0),          # one k-step exactly
    "one_tap_more": Shape(128, 65, 7, 65 + 7 * 33 + 3, 2, 7),    # one tap into the second step, a hop off the 16-byte path
    "hop_one": Shape(16, 16, 1, 16 + 300, 2, 0),                 # W = n_fft = 16, H = 1
    "common": Shape(512, 400, 160, 4000, 4, 80),                 # 25 ms / 10 ms at 16 kHz, 80 mels
}


def shape_inputs(name):
    """-> (rows int16 [R, T], window float32 [W], filters or None)"""
    s = SHAPES[name]
    rng = np.random.default_rng(sum(name.encode()))
    rows = rng.integers(-32768, 32768, size=(s.rows, s.T)).astype(np.int16)
    rows[-1] //= 64  # a quiet row
    filters = mel_filters_oracle(16000, s.n_fft, s.mels) if s.mels else None
    return rows, so.hann(s.W), filters


def mel_filters_oracle(rate, n_fft, n_mels):
    return so.mel_filters(rate, n_fft, n_mels)


LIMIT_FFT, LIMIT_H = 4096, 160


def limit_inputs():
    """n_fft = W = 4096 with a flat window of 1.99 (q = 14, every coefficient near the bound) and one rail row of T = 4096 + 160
    whose signs follow bin 5's cos column: frame 0's Re[5] lies next to 2^42 -> (row [1, T], window, q, cq, sq)"""
    window = np.full(LIMIT_FFT, 1.99, dtype=np.float32)
    q, cq, sq = so.quantise(window, LIMIT_FFT)
    sign = np.where(cq[:, 5] >= 0, 32767, -32768).astype(np.int16)
    row = np.concatenate([sign, sign[:LIMIT_H]])[None, :]
    return row, window, q, cq, sq
