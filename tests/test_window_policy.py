"""Window decode on the CPU: the launch arithmetic of aad_launch_policy.h (plan_window_decode, window_blocks_spanned,
window_blocks_at), built with g++ into tests/window_policy_driver.cpp, and the numpy restatement of the definition
(tests/window_oracle.py) that the GPU tests compare against, checked against itself on edge tables.

Lanes: one per (window, block-in-window, channel).  A window of T frames starting `phase` frames into a block of spb frames touches
(phase + T - 1) // spb + 1 blocks, at most K = ceil((T - 1) / spb) + 1 (phase spb - 1); lanes = N * K * C, workgroup and occupancy
cap as the per-lane dense decoder's, the grid capped at 2^20 workgroups (the kernel walks the rest grid-stride)."""
import os
import subprocess

import numpy as np
import pytest

from window_oracle import window_expected

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "aad_amd", "csrc")
MI355X = (256, 163840)
SMALL = (32, 65536)
MAX_GRID = 1 << 20


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("window_policy") / "window_policy_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "window_policy_driver.cpp")], check=True)
    return str(exe)


def run(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


def touched(phase, frames, spb):
    """blocks whose frames [b spb, (b + 1) spb) meet [phase, phase + frames), counted block by block"""
    b = np.arange(0, (phase + frames) // spb + 3, dtype=np.int64)
    return int(np.count_nonzero((b * spb < phase + frames) & ((b + 1) * spb > phase)))


@pytest.mark.parametrize("spb", [1, 2, 7, 64, 1020])
def test_blocks_spanned_at_every_phase(driver, spb):
    lengths = {1, max(spb - 1, 1), spb, spb + 1}
    for k in (2, 3, 7):
        lengths |= {k * spb - 1, k * spb, k * spb + 1}
    lengths = sorted(lengths)
    for frames, line in zip(lengths, run(driver, ["S %d %d" % (t, spb) for t in lengths])):
        got = [int(v) for v in line.split()]
        kmax, per_phase = got[0], got[1:]
        want = [touched(ph, frames, spb) for ph in range(spb)]
        assert per_phase == want, (spb, frames)
        assert kmax == max(want) == -(-(frames - 1) // spb) + 1, (spb, frames)
    assert run(driver, ["S 0 %d" % spb])[0].split()[0] == "0"


def expected_plan(device, pad, windows, frames, channels, bits, spb, lds_dense):
    cus, lds_per_cu = device
    k = -(-(frames - 1) // spb) + 1
    lanes = windows * k * channels
    wg = 64 if lanes <= cus * 256 else 256
    grid = min(-(-lanes // wg), MAX_GRID) if lanes else 0
    lds = 0
    if wg == 256 and lanes:
        if pad >= 0:
            lds = pad
        elif (channels == 1 or (channels == 2 and bits != 4)) and lanes >= cus * 256:
            lds = lds_per_cu // 2 - lds_dense
    return "1 %d %d %d %d %d %d" % (k, wg if lanes else 0, grid, lds, lanes, windows * channels * frames)


ROWS = [  # windows frames channels bits spb decode_lds_pad
    (4096, 48000, 2, 4, 992, -1),   # the chip-filling measurement: stereo 4-bit keeps its occupancy
    (64, 48000, 2, 4, 992, -1),     # the latency measurement: one-wave workgroups
    (4096, 48000, 1, 4, 2012, -1),  # mono: the occupancy cap
    (4096, 48000, 2, 3, 1316, -1),
    (4096, 48000, 8, 2, 500, -1),   # any-channel: keeps its occupancy
    (1, 1, 1, 4, 2012, -1),
    (3, 1, 2, 2, 5, 4096),
    (1000, 992, 2, 4, 992, 0),      # T = spb: two blocks per window
    (1000, 993, 2, 4, 992, -1),
    (1000, 994, 2, 4, 992, -1),     # T = spb + 2: three
    (0, 48000, 2, 4, 992, -1),      # no windows: nothing to launch
    (1 << 28, 16, 8, 4, 100, -1),   # 2^32 lanes: grid capped
    (1 << 40, 1, 1, 3, 7, 1024),
]


@pytest.mark.parametrize("device", [MI355X, SMALL], ids=["mi355x", "32cu_64k"])
def test_lane_count_and_grid(driver, device):
    lds_dense = int(run(driver, ["L"])[0])
    lines = ["W %d %d %d %d %d %d %d %d" % (device[0], device[1], pad, n, t, c, b, spb) for n, t, c, b, spb, pad in ROWS]
    for row, got in zip(ROWS, run(driver, lines)):
        n, t, c, b, spb, pad = row
        assert got == expected_plan(device, pad, n, t, c, b, spb, lds_dense), row
    # the rows the MI355X actually measures, spelled out
    got = run(driver, ["W 256 163840 -1 4096 48000 2 4 992", "W 256 163840 -1 64 48000 2 4 992"])
    assert got == ["1 50 256 1600 0 409600 393216000", "1 50 64 100 0 6400 6144000"]


def test_overflow_refused(driver):
    rows = [
        ("W 256 163840 -1 %d 2 2 4 992" % (1 << 62), "0"),             # N C T = 2^64 elements
        ("W 256 163840 -1 %d 2 1 4 992" % (1 << 61), "0"),             # 2^62 elements: 2^64 float32 bytes
        ("W 256 163840 -1 %d 1 1 4 992" % (1 << 60), "1"),             # 2^62 bytes: fine
        ("W 256 163840 -1 %d 4294967295 8 4 5" % (1 << 30), "0"),      # lanes and elements past 2^64
        ("W 256 163840 -1 %d 1 8 4 992" % ((1 << 64) - 1), "0"),
        ("W 256 163840 -1 1 0 2 4 992", "0"),                          # T = 0
    ]
    for line, ok in rows:
        assert run(driver, [line])[0].split()[0] == ok, line


def _decoded(seed, lengths, channels):
    rng = np.random.default_rng(seed)
    return [rng.integers(-32768, 32768, size=(n, channels), dtype=np.int64).astype(np.int16) for n in lengths]


def test_definition_restatement_on_edge_tables():
    channels = 3
    decoded = _decoded(5, [0, 1, 17, 1000, 4099], channels)
    n = 1000
    d = decoded[3]
    edge = [(3, 0), (3, 1), (3, 999), (3, 1000), (3, 10 ** 12), (3, -1), (5, 0), (-1, 0), (2, 16), (0, 0), (4, 4000)]
    for frames in (1, 7, 64, 1000, 1001, 5000):
        got = window_expected(decoded, edge, frames, channels)
        assert got.shape == (len(edge), channels, frames) and got.dtype == np.int16
        for w, (s, f) in enumerate(edge):
            if s < 0 or s >= len(decoded) or f < 0 or f >= decoded[s].shape[0]:
                assert not got[w].any(), (frames, s, f)  # bad stream, past the end, wrapped int64: zeros
                continue
            src = decoded[s]
            m = min(frames, src.shape[0] - f)
            assert np.array_equal(got[w, :, :m], src[f:f + m].T)
            assert not got[w, :, m:].any()
        # float32: int16 / 32768, bit for bit
        f32 = window_expected(decoded, edge, frames, channels, np.float32)
        assert f32.dtype == np.float32 and np.array_equal(f32.view(np.uint32), (got.astype(np.float32) * np.float32(1 / 32768)).view(np.uint32))
    # the whole stream is one window; adjacent windows tile a longer one
    assert np.array_equal(window_expected(decoded, [(3, 0)], n, channels)[0], d.T)
    long = window_expected(decoded, [(4, 100)], 3000, channels)[0]
    parts = window_expected(decoded, [(4, 100), (4, 1100), (4, 2100)], 1000, channels)
    assert np.array_equal(np.concatenate(list(parts), axis=1), long)
    # crossing the end: the same as the stream's tail then zeros
    tail = window_expected(decoded, [(4, 4000)], 200, channels)[0]
    assert np.array_equal(tail[:, :99], decoded[4][4000:].T) and not tail[:, 99:].any()
