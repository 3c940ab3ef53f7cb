"""The mix kernels of the spectrogram stage (aad_amd/csrc/aad_spectrogram_mix.hip, namespace aad::spectrum_mix), one record per
instantiation, and the inputs of the cases of tests/test_gpu_spectrogram_mix.py, on which tests/test_spectrogram_mix_host.py runs
the numpy mutants and the witness census.  tests/test_spectrogram_mix_kernel_census.py holds the built library to exactly the
records.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import os
import re
import subprocess
from collections import namedtuple

import numpy as np

from kernel_names import ARG

import spectrogram_matrix as sm
import spectrogram_mix_oracle as mo

GPU_FILE = "test_gpu_spectrogram_mix.py"
HERE = os.path.dirname(os.path.abspath(__file__))

Cell = namedtuple("Cell", "kernel args case")

# _ZN3aad12spectrum_mix <length> <name> I <arguments> E E: spectrogram_matrix.NAME reads "12spectrum_mix..." as no name of its own
NAME = re.compile(rb"_ZN3aad12spectrum_mix(\d+)([a-z][a-z0-9_]*_kernel)(?:I((?:L[ib]n?\d+E)+)E)?E")


def kernels_in(data):
    """bytes -> the set of (kernel, template arguments) among the mangled names of aad::spectrum_mix kernels in them"""
    found = set()
    for m in NAME.finditer(data):
        name = m.group(2)
        if int(m.group(1)) != len(name):
            continue
        found.add((name.decode(), tuple(-int(v) if neg else int(v) for _, neg, v in ARG.findall(m.group(3) or b""))))
    return found


def cells():
    """MEL false: the power spectrum of the mix from the lanes; MEL true: the filterbank behind the hand-off buffer"""
    return [Cell("spectrum_mix_rows_kernel", (0,), "test_small_every_edge"), Cell("spectrum_mix_rows_kernel", (1,), "test_small_every_edge")]


# ---- the header through g++ ----------------------------------------------------------------------------------------------------------

def build_driver(directory):
    exe = os.path.join(str(directory), "spectrogram_mix_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", sm.CSRC, "-o", exe, os.path.join(HERE, "spectrogram_mix_driver.cpp")],
                   check=True)
    return exe


# ---- the small case: every edge ------------------------------------------------------------------------------------------------------

SMALL_HOPS = (16, 37)  # one per staging mode of spectrum_geometry
SMALL_TILE_FRAMES = 256  # of both hops at W 80; the tests hold it against the header through the driver
ROWS_PER_GAIN = 2
PITCH_EXTRA = (1, 37)  # a at pitch T + 1, b at pitch T + 37
PARITIES = ((1, 0), (0, 1))  # of the two row pointers
F32 = np.float32

# (gain_a, gain_b) per group, None for NULL tables
GAINS = {
    "null": (None, None),
    "halves": (np.array([0.5, 0.5], dtype=F32), np.array([0.5, 0.5], dtype=F32)),          # ties with even and odd floors
    "signed": (np.array([-0.75, 1.0], dtype=F32), np.array([-1.3, 0.7], dtype=F32)),        # 0.7f: both rails clip in group 1
}
WITNESS_GAINS = (F32(-0.75), F32(-1.3))  # group 0 of "signed", whose row 0 holds the planted witnesses
WITNESS_AT = (5, 1001, 2002, 3003)


def fma_witnesses(ga, gb, count):
    """(a, b) pairs whose staged sample a fused multiply-add changes, the first `count` of a fixed search order: random draws
    witness it too rarely to be relied on"""
    b = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    found = []
    for a in range(-32001, 32768, 977):
        av = np.full(b.shape, a, dtype=np.int16)
        differ = np.flatnonzero(mo.mix_element(ga, av, gb, b, True) != mo.mix_element(ga, av, gb, b, True, "fma"))
        found += [(a, int(b[i])) for i in differ[:1]]
        if len(found) >= count:
            return found[:count]
    raise AssertionError("no fused multiply-add witness found")


EDGE_L, EDGE_BEFORE = 101, 51  # the span across the tile boundary: its length, and how much of it lies below the boundary


def small_spans(H, T):
    """the span tables of the small case, (L, o) per group as Python ints; None: a NULL table"""
    boundary = SMALL_TILE_FRAMES * H  # the first sample of the second tile's first frame
    assert boundary - EDGE_BEFORE + EDGE_L < T
    return {
        "null": None,
        "whole": [(T, 0), (T, 0)],
        "edges": [(EDGE_L, boundary - EDGE_BEFORE), (2 ** 64 - 1, T)],   # odd o, odd L across the tile boundary; Le = 0 through o >= T
        "clipped": [(2 ** 63, 3), (0, 5)],                    # L past the row: Le = T - 3; L = 0
    }


def small_rows(H):
    """-> (T, a int16 [4, T], b int16 [4, T]): a the hand-made rows (noise, -32768, alternating rails, silence), b noise with the
    planted witnesses, +32767, alternating rails in phase with a's, noise"""
    T = sm.small_frames(H, SMALL_TILE_FRAMES)
    a = sm.hand_made_rows(T)
    rng = np.random.default_rng(23)
    b = np.zeros((4, T), dtype=np.int16)
    b[0] = rng.integers(-32768, 32768, size=T)
    b[1] = 32767
    b[2] = a[2]
    b[3] = rng.integers(-32768, 32768, size=T)
    for at, (wa, wb) in zip(WITNESS_AT, fma_witnesses(WITNESS_GAINS[0], WITNESS_GAINS[1], len(WITNESS_AT))):
        a[0, at], b[0, at] = wa, wb
    return T, a, b


def small_cases(H):
    """every (gains name, spans name) of the small case at hop H -> (T, a, b, [(label, gain_a, gain_b, spans)])"""
    T, a, b = small_rows(H)
    spans = small_spans(H, T)
    cases = [("%s/%s" % (g, s), GAINS[g][0], GAINS[g][1], spans[s]) for g in GAINS for s in spans]
    return T, a, b, cases


def span_table(spans):
    """(L, o) Python ints per group -> the int64 [G, 2] table a torch tensor holds, values past 2^63 wrapped"""
    return np.array(spans, dtype=np.uint64).view(np.int64).reshape(-1, 2)


def special_gain_case():
    """NaN and infinite gains over one short batch: -> (a, b [6, T], gain_a, gain_b [6]); rows_per_gain 1"""
    T = sm.SMALL_W + 16 * 5
    rng = np.random.default_rng(31)
    a = rng.integers(-32768, 32768, size=(6, T)).astype(np.int16)
    b = rng.integers(-32768, 32768, size=(6, T)).astype(np.int16)
    a[:, 7], b[:, 9] = 0, 0  # inf * 0 is a NaN: an element 0 among rails
    a[4, 11], b[4, 11] = 5, 5  # inf - inf
    inf, nan = np.inf, np.nan
    gain_a = np.array([nan, 1.0, inf, -inf, inf, 1.0], dtype=F32)
    gain_b = np.array([1.0, nan, 1.0, 0.5, -inf, inf], dtype=F32)
    return a, b, gain_a, gain_b
