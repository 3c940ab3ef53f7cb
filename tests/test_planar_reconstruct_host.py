"""Planar reconstruct on the CPU (include/aad_hip.h "planar reconstruct"): the library exports the two entry points, the launch
policy never plans the dual trial search or the byte ring for a reconstruct plan (aad_amd/csrc/aad_launch_policy.h
plan_reconstruct_encode - the kernels that write the decoded rows exist for neither), and the output-layout check
(planar_output_ok) refuses overlapping rows, bad fields and 64-bit overflow, through tests/planar_reconstruct_host_driver.cpp built
with g++ against the policy header."""
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
