"""Planar reconstruct on the CPU (include/aad_hip.h "planar reconstruct"): the library exports the two entry points, the launch
policy never plans the dual trial search or the byte ring for a reconstruct plan (aad_amd/csrc/aad_launch_policy.h
plan_reconstruct_encode - the kernels that write the decoded rows exist for neither), and the output-layout check
(planar_output_ok) refuses overlapping rows, bad fields and 64-bit overflow, and a plan's per-lane output bases
(aad_amd/csrc/aad_segments.h reconstruct_output_bases), read off the chain table, are where the segment arithmetic puts them,
through tests/planar_reconstruct_host_driver.cpp built with g++ against the policy and segment headers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
I16, F32 = 0, 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("planar_reconstruct") / "planar_reconstruct_host_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o",
                    str(exe), os.path.join(ROOT, "tests", "planar_reconstruct_host_driver.cpp")], check=True)
    return str(exe)


def test_library_exports_the_two_entry_points():
    from aad_amd.capi import HIP_SYMBOLS, load_library
    lib = load_library()
    for name in ("AADHip_PlanarReconstructPlanCreate", "AADHip_PlanarReconstructPlanRun"):
        assert name in HIP_SYMBOLS
        getattr(lib, name)


def test_reconstruct_plans_never_take_the_dual_search_or_the_ring(driver):
    batches, rec_dual, rec_ring, enc_dual, enc_ring = (int(v) for v in subprocess.run([driver, "policy"], check=True, capture_output=True,
                                                                                       text=True).stdout.split())
    assert batches > 10000
    assert enc_dual > 0 and enc_ring > 0, "the sweep must reach the shapes where an encode plan picks them"
    assert rec_dual == 0, "a reconstruct plan chose the dual trial search"
    assert rec_ring == 0, "a reconstruct plan chose the byte ring"


def check(driver, cases):
    lines = ["%d %d %d %d %d %d %s" % (ch, t, r, ss, cs, len(ns), " ".join(str(v) for v in ns)) for ch, t, r, ss, cs, ns in cases]
    out = subprocess.run([driver, "output"], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(cases)
    return out


def test_output_layout_accepts_tight_and_loose_rows(driver):
    cases = [(2, F32, 0, 2 * 100, 100, [100, 50, 100]),       # contiguous [N, C, T]
             (2, I16, 0, 1000, 300, [100, 7]),                 # gaps everywhere
             (1, I16, 0, 100, 0, [100, 3]),                    # mono: channel_stride unused
             (8, F32, 0, 8 * 64, 64, [64] * 5),
             (3, I16, 0, 0, 10, [10]),                         # one stream: stream_stride unused
             (2, F32, 0, 123, 55, [])]                         # no streams
    assert check(driver, cases) == ["ok"] * len(cases)


def test_output_layout_refuses_bad_fields_and_overlap(driver):
    cases = [(2, 2, 0, 200, 100, [100]),                       # unknown sample type
             (2, -1, 0, 200, 100, [100]),
             (2, F32, 1, 200, 100, [100]),                     # reserved
             (2, I16, 0, 400, 99, [100, 10]),                  # channel rows overlap
             (2, I16, 0, 199, 100, [100, 100]),                # stream i's last row runs into stream i + 1's first
             (3, F32, 0, 250, 100, [50, 100]),                 # (C - 1) cs + longest = 300 > 250
             (1, I16, 0, 99, 0, [100, 100])]                   # mono rows overlap
    assert check(driver, cases) == ["refused"] * len(cases)


def test_output_layout_refuses_64_bit_overflow(driver):
    big = 1 << 63
    cases = [(2, I16, 0, 200, big, [100]),                     # (C - 1) cs + n: fits in elements, not in int16 bytes
             (3, I16, 0, 200, big, [100]),                     # (C - 1) cs overflows elements
             (2, I16, 0, big, 100, [100, 100, 100]),           # (N - 1) ss overflows
             (2, F32, 0, (1 << 62) - 1, 100, [100, 100]),      # element offsets fit, float32 bytes do not
             (1, I16, 0, (1 << 64) - 50, 0, [100, 100])]       # ss + n past 2^64
    assert check(driver, cases) == ["refused"] * len(cases)
    ok = [(2, I16, 0, 200, (1 << 62) - 200, [100]), (2, I16, 0, (1 << 62), 100, [100, 100])]
    assert check(driver, ok) == ["ok", "ok"]


def test_output_bases_follow_the_chain_table(driver):
    """Lane (i, s) - stream i, segment s of L blocks with W warm-up blocks - writes its first frame, warm-up included, at
    i * stream_stride + (s L - min(W, s L)) * spb; the segment arithmetic is written out here, the library reads the chain table."""
    batches = [[1], [5], [63], [64], [65], [1000], [64 * 7], [64 * 7 + 1],
               [3, 700, 64, 1, 129, 5000, 64 * 12],          # ragged, streams shorter than a block among them
               [10, 20, 30], [4097] * 4]
    cases = []
    for spb in (64, 100):
        for L in (1, 2, 3, 8, 1000):
            for W in (0, 1, 2, 5, 9, 2000):                  # W = 0, W < L, W = L, W > L
                for ns in batches:
                    cases.append((spb, L, W, max(ns) + 17, ns))
        for ns in batches:
            cases.append((spb, 0, 0, max(ns), ns))           # unsegmented: one lane per stream
    assert any(W > L for _, L, W, _, _ in cases) and any(min(ns) < spb for spb, _, _, _, ns in cases)
    lines = ["%d %d %d %d %d %s" % (spb, L, W, ss, len(ns), " ".join(str(v) for v in ns)) for spb, L, W, ss, ns in cases]
    out = subprocess.run([driver, "bases"], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (spb, L, W, ss, ns), line in zip(cases, out):
        want = []
        for i, n in enumerate(ns):
            if L == 0:
                want.append(i * ss)
                continue
            blocks = -(-n // spb)
            for s in range(-(-blocks // L)):
                want.append(i * ss + (s * L - min(W, s * L)) * spb)
        assert [int(v) for v in line.split()] == want, (spb, L, W, ss, ns)
