"""Window decode statistics on the CPU (include/aad_hip.h, AADHip_WindowDecodePlanRunStats): the numpy restatement of the
definition (tests/window_stats_oracle.py) at its own corners, the table-size policy of aad_launch_policy.h (window_stats_table,
built with g++ into tests/window_stats_policy_driver.cpp) and the export of the entry point."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from window_stats_oracle import channel_mix_stats_expected, stats_of_rows, window_counts, window_stats_expected

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "aad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("window_stats_policy") / "window_stats_policy_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "window_stats_policy_driver.cpp")], check=True)
    return str(exe)


def run(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [tuple(int(v) for v in line.split()) for line in out]


# ---- the oracle's own corners -------------------------------------------------------------------------------------------------
def test_oracle_corners():
    rng = np.random.default_rng(3)
    d0 = rng.integers(-32768, 32768, size=(1000, 2), dtype=np.int64).astype(np.int16)
    d1 = np.full((40, 2), -32768, dtype=np.int16)
    d2 = np.zeros((0, 2), dtype=np.int16)  # a stream without frames
    decoded = [d0, d1, d2]
    windows = [(0, 0), (1, 0), (1, 39), (1, 40), (3, 0), (-1, 0), (0, -1), (0, 999), (0, 990), (2, 0), (0, 1 << 40)]
    frames = 16
    got = window_stats_expected(decoded, windows, frames, 2)
    assert got.shape == (len(windows), 2, 4) and got.dtype == np.int64 and (got >= 0).all()
    # an ordinary row, against python integers
    v = [int(x) for x in d0[:16, 1]]
    assert got[0, 1].tolist() == [sum(x * x for x in v), sum(abs(x) for x in v), max(abs(x) for x in v), 16]
    # a row of -32768: |v| = 32768 is reachable, sixteen of them are 2^34
    assert got[1, 0].tolist() == [16 << 30, 16 << 15, 32768, 16] and got[1, 0, 0] == 1 << 34
    # first_frame = num_samples - 1: one frame
    assert got[2, 0].tolist() == [1 << 30, 32768, 32768, 1] and got[7, :, 3].tolist() == [1, 1]
    assert got[8, :, 3].tolist() == [10, 10]
    # first_frame = num_samples, a stray window, wrapped stream and first_frame, an empty stream, a huge first_frame: empty rows
    for w in (3, 4, 5, 6, 9, 10):
        assert not got[w].any(), w
    assert window_counts([1000, 40, 0], windows, frames).tolist() == [16, 16, 1, 0, 0, 0, 0, 1, 10, 0, 0]
    # count comes from the lengths, not from the rows: a truncated image's decode has zeros where the table still has frames
    cut = [np.concatenate([d0[:500], np.zeros((500, 2), np.int16)]), d1, d2]
    t = window_stats_expected(cut, [(0, 400), (0, 600)], 200, 2, lengths=[1000, 40, 0])
    assert t[:, :, 3].tolist() == [[200, 200], [200, 200]] and not t[1, :, :3].any() and t[0, 0, 0] > 0
    # T = 0 rows: max_abs is 0 when nothing contributes
    assert not stats_of_rows(np.zeros((2, 3, 0), np.int16), [0, 0]).any()
    # the largest sums stay inside int64: 2^62 at T = 2^32 would; here the per-sample bound
    assert stats_of_rows(np.full((1, 1, 4096), -32768, np.int16), [4096])[0, 0].tolist() == [4096 << 30, 4096 << 15, 32768, 4096]


def test_oracle_channel_mix_rules():
    lr = np.array([[-32768, -32768], [32767, 32767], [-5, 2], [100, -101], [7, 8]], dtype=np.int16)  # sums -65536 65534 -3 -1 15
    mono = np.array([[-32768], [5], [-7]], dtype=np.int16)
    decoded = [lr, mono]
    down = channel_mix_stats_expected(decoded, [(0, 0), (1, 0), (2, 0)], 8, 1)
    mix = [-32768, 32767, -2, -1, 7]  # the floor of the mean
    assert down[0, 0].tolist() == [sum(v * v for v in mix), sum(abs(v) for v in mix), 32768, 5]
    assert down[1, 0].tolist() == [(1 << 30) + 25 + 49, 32768 + 12, 32768, 3] and not down[2].any()
    up = channel_mix_stats_expected(decoded, [(1, 1), (0, 2)], 2, 2)
    assert up[0, 0].tolist() == up[0, 1].tolist() == [74, 12, 7, 2]  # a mono stream in two rows: two equal records
    assert up[1, 0].tolist() == [25 + 10000, 105, 100, 2] and up[1, 1].tolist() == [4 + 10201, 103, 101, 2]


# ---- the table of a run --------------------------------------------------------------------------------------------------------
def test_table_size_and_refusals(driver):
    rows = [
        ("T 0 2 0", (1, 0)),                                   # no windows: nothing to write, any pointer
        ("T 0 2 4", (1, 0)),
        ("T 1 1 4096", (1, 32)),
        ("T 4096 2 4096", (1, 4096 * 2 * 32)),
        ("T 512 8 8", (1, 512 * 8 * 32)),
        ("T 1 1 0", (0, 32)),                                  # null with windows
        ("T 1 2 4100", (0, 64)),                               # not 8-byte aligned
        ("T 1 2 4097", (0, 64)),
        ("T 7 1 %d" % ((1 << 48) + 8), (1, 224)),
        ("T %d 1 4096" % (1 << 58), (1, 1 << 63)),
        ("T %d 1 4096" % (1 << 59), (0, 0)),                   # N C 32 = 2^64 ...
        ("T %d 2 4096" % (1 << 58), (0, 0)),
        ("T %d 8 4096" % ((1 << 64) - 1), (0, 0)),             # N C itself overflows
    ]
    got = run(driver, [line for line, _ in rows])
    for (line, want), g in zip(rows, got):
        assert g == want, line


def test_table_overflows_where_short_rows_do_not(driver):
    """T < 8: N C T 4 bytes of float32 rows fit 64 bits where N C 32 bytes of records do not - plan_window_decode accepts the run,
    window_stats_table refuses it"""
    policy = os.path.join(os.path.dirname(driver), "window_policy_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", policy, os.path.join(HERE, "window_policy_driver.cpp")], check=True)
    for frames in (1, 2, 4, 7):
        n = (1 << 59)
        assert n * frames * 4 < 1 << 64 <= n * 32
        out = subprocess.run([policy], input="W 256 163840 -1 %d %d 1 4 992\n" % (n, frames), check=True, capture_output=True,
                             text=True).stdout.split()
        assert out[0] == "1", frames
        assert run(driver, ["T %d 1 4096" % n])[0] == (0, 0)
    assert run(driver, ["T %d 1 4096" % ((1 << 59) - 1)])[0] == (1, ((1 << 59) - 1) * 32)


# ---- the export ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point():
    from aad_amd.capi import AADApiResult, HIP_SYMBOLS, load_library
    lib = load_library()
    assert "AADHip_WindowDecodePlanRunStats" in HIP_SYMBOLS
    fn = lib.AADHip_WindowDecodePlanRunStats
    assert len(fn.argtypes) == 8 and fn.restype is C.c_int
    assert fn(None, None, 0, None, 1, 0, None, None) == AADApiResult.INVALID_ARGUMENT  # no plan: refused before any device is touched
    text = open(os.path.join(ROOT, "include", "aad_hip.h")).read()
    assert "AADHip_WindowDecodePlanRunStats(" in text
    for word in ("sum_sq", "max_abs", "count", "(L + R) >> 1", "statistics only"):
        assert word in text[text.index("Window decode with exact per-row level statistics"):text.index("AADHip_WindowDecodePlanRunStats(")]


def test_level_dbfs():
    torch = pytest.importorskip("torch")
    from aad_amd.engine import level_dbfs, rmse
    stats = torch.tensor([[[1 << 30, 1 << 15, 32768, 1], [0, 0, 0, 100], [0, 0, 0, 0], [16 << 28, 16 << 14, 16384, 16]]], dtype=torch.int64)
    got = level_dbfs(stats)
    assert got.dtype == torch.float64 and got.shape == (1, 4)
    assert got[0, 0].item() == 0.0 and got[0, 1].item() == float("-inf") and got[0, 2].item() == float("-inf")
    assert abs(got[0, 3].item() - 20 * np.log10(0.5)) < 1e-12
    assert torch.equal(got[0, [0, 3]], 20.0 * (rmse(stats)[0, [0, 3]] / 32768.0).log10())
