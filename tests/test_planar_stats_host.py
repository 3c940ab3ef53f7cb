"""Planar reconstruct statistics on the CPU (include/aad_hip.h "planar reconstruct statistics"): struct AADHipRowStats is four
uint64 (32 bytes) for a C compiler and for ctypes, so that a torch int64 [N, C, 4] tensor is the table; the built library exports
AADHip_PlanarReconstructPlanRunStats and HIP_SYMBOLS names it; the chains of a segmented plan add into the records of their own
stream (aad_amd/csrc/aad_segments.h chain_streams, through tests/planar_stats_host_driver.cpp built with g++)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aad_amd", "csrc")

SNIPPET = r"""
#include <stddef.h>
#include <stdio.h>
#include "aad_hip.h"
int main(void)
{
  printf("%u %u %u %u %u\n", (unsigned)sizeof(struct AADHipRowStats), (unsigned)offsetof(struct AADHipRowStats, sum_sq),
         (unsigned)offsetof(struct AADHipRowStats, sum_abs), (unsigned)offsetof(struct AADHipRowStats, max_abs),
         (unsigned)offsetof(struct AADHipRowStats, count));
  return 0;
}
"""


def test_row_stats_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(SNIPPET)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split() == ["32", "0", "8", "16", "24"]


def test_row_stats_layout_in_ctypes():
    from aad_amd.capi import AADHipRowStats
    assert C.sizeof(AADHipRowStats) == 32
    assert [getattr(AADHipRowStats, f).offset for f in ("sum_sq", "sum_abs", "max_abs", "count")] == [0, 8, 16, 24]
    assert all(getattr(AADHipRowStats, f).size == 8 for f in ("sum_sq", "sum_abs", "max_abs", "count"))


def test_library_exports_the_entry_point():
    from aad_amd.capi import AADApiResult, HIP_SYMBOLS, load_library
    lib = load_library()
    assert "AADHip_PlanarReconstructPlanRunStats" in HIP_SYMBOLS
    fn = lib.AADHip_PlanarReconstructPlanRunStats
    assert len(fn.argtypes) == 6 and fn.restype is C.c_int
    assert fn(None, None, None, None, None, None) == AADApiResult.INVALID_ARGUMENT  # no plan: refused before any device is touched


def test_chains_add_into_their_own_stream(tmp_path):
    exe = tmp_path / "planar_stats_host_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o",
                    str(exe), os.path.join(ROOT, "tests", "planar_stats_host_driver.cpp")], check=True)
    cases = []
    for spb in (64, 100):
        for L in (1, 3, 16, 1000):
            for W in (0, 1, 4, 2000):
                for ns in ([1], [64], [65], [3, 700, 64, 1, 129, 5000, 64 * 12], [4097] * 4, [10, 20, 30]):
                    cases.append((spb, L, W, ns))
    lines = ["%d %d %d %d %s" % (spb, L, W, len(ns), " ".join(str(v) for v in ns)) for spb, L, W, ns in cases]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (spb, L, W, ns), line in zip(cases, out):
        want = []
        for i, n in enumerate(ns):
            blocks = -(-n // spb)
            want += [i] * -(-blocks // L)  # one chain per segment of L blocks, whatever the warm-up
        assert [int(v) for v in line.split()] == want, (spb, L, W, ns)
