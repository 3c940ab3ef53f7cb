"""The launch policy under a SIMD role (AAD_HIP_OPTION_SIMD_ROLE; aad_amd/csrc/aad_launch_policy.h plan_simd_role), on the CPU:
tests/simd_role_policy_driver.cpp is built with g++ against the header and prints the plan of every row.

 - role off gives the plans of tests/test_launch_policy.py's tables exactly (every row of both devices), and no role fields;
 - under a role the quad encoder of a lane-starved batch runs four-wave workgroups on the SAME grid (one per sixteen recurrences),
   up to one workgroup per CU: 4096 recurrences on the MI355X, 4097 keep one-wave workgroups.  The dual trial search and the
   dense encoders never take a role; the planar reconstruct plan (single-layout search) does;
 - the split decoder with its residuals in LDS takes the role's SIMD and dynamic LDS rows that are a function of the block
   geometry alone - coded samples rounded up to a chunk of 16, + 4 dwords, sixteen rows - whatever the batch size; blocks above
   2048 coded samples keep the scratch path (no dynamic LDS) and still elect their recurrence wave while there is at most one
   workgroup per CU; past the split decoder's limits (4097 recurrences: scratch rows on 257 workgroups; 8193: dense) a role is
   ignored."""
import os
import subprocess

import pytest

from test_launch_policy import CSRC, HERE, MI355X, MI355X_TABLE, SMALL, SMALL_TABLE


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("role_policy") / "simd_role_policy_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "simd_role_policy_driver.cpp")], check=True)
    return str(exe)


def run(driver, device, rows, role):
    """rows: "K knobs | batch" as in test_launch_policy -> the driver's output lines"""
    lines = []
    for batch in rows:
        knobs, fields = batch.split(" | ")
        kind, rest = knobs.split(" ", 1)
        lines.append("%s %d %d %s %d %s" % (kind, device[0], device[1], rest, role, fields))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(rows)
    return out


@pytest.mark.parametrize("device,table", [(MI355X, MI355X_TABLE), (SMALL, SMALL_TABLE)], ids=["mi355x", "32cu_64k"])
def test_role_off_is_todays_plan(driver, device, table):
    rows = [r.split(" -> ") for r in table.strip().splitlines()]
    got = run(driver, device, [b for b, _ in rows], -1)
    for (batch, want), g in zip(rows, got):
        tail = " 0" if batch[0] == "E" else " 0 0"
        assert g == want + tail, (batch, want, g)


K = "0 0 1 -1 -1 0"  # auto mapping, dual trial lanes, ring by policy, pads by policy


@pytest.mark.parametrize("role", [0, 1, 2, 3])
def test_quad_encoder_role(driver, role):
    rows = ["E %s | 4 2 1000 0 1024 1" % K,   # the headline: 2000 recurrences, 125 workgroups
            "E %s | 4 1 1 0 1024 1" % K,
            "E %s | 3 1 4096 0 1024 1" % K,   # one workgroup per CU
            "E %s | 3 1 4097 0 1024 1" % K,   # 257 workgroups: no role
            "E %s | 4 2 8192 0 1024 1" % K,
            "E %s | 4 2 1000 2 1024 1" % K,   # dual trial search
            "E 0 1 1 -1 -1 0 | 4 2 1000 2 1024 1",  # single-layout trial search: the quad kernel
            "R %s | 4 2 1000 2 1024 0" % K,   # planar reconstruct: always the single layout
            "E %s | 4 1 16385 0 1024 1" % K,  # dense
            "E 1 0 1 -1 -1 0 | 4 2 1000 0 1024 1"]  # dense forced
    r = role + 1
    assert run(driver, MI355X, rows, role) == [
        "quad 0 256 125 0 0 0 %d" % r,
        "quad 0 256 1 0 0 0 %d" % r,
        "quad 0 256 256 0 0 0 %d" % r,
        "quad 0 64 257 0 0 0 0",
        "quad 0 64 1024 0 0 0 0",
        "quad-dual 1 128 125 0 1088 3264000 0",
        "quad 1 256 125 0 0 0 %d" % r,
        "quad 1 256 125 0 0 0 %d" % r,
        "dense 0 64 257 0 0 0 0",
        "dense 0 64 32 0 0 0 0"]
    # a 32-CU device: 512 recurrences
    assert run(driver, SMALL, ["E %s | 4 1 512 0 1024 1" % K, "E %s | 4 1 513 0 1024 1" % K], role) == [
        "quad 0 256 32 0 0 0 %d" % r, "quad 0 64 33 0 0 0 0"]


def lds_of(coded):
    row = (coded + 15) // 16 * 16 + 4
    return row, 16 * row * 4


@pytest.mark.parametrize("role", [0, 1, 2, 3])
def test_split_decoder_role(driver, role):
    r = role + 1
    # blocks streams channels bits samples_per_block block_size pcm_aligned16 pcm_base_aligned16 code_phase_uniform stream_stores
    geometries = [(2, 4, 992, 1024), (1, 4, 2016, 1024), (2, 3, 1320, 1026), (2, 2, 1980, 1024), (1, 4, 5, 1024), (2, 4, 20, 1024),
                  (1, 2, 2052, 530)]
    for ch, bits, spb, bs in geometries:
        row, lds = lds_of(spb - 4)
        for streams in (1, 1000 // ch, 4096 // ch):
            got = run(driver, MI355X, ["D %s | %d %d %d %d %d %d 1 1 1 1" % (K, streams, streams, ch, bits, spb, bs)], role)[0]
            grid = (streams * ch + 15) // 16
            assert got == "split-lds 0 1024 %d %d 0 0 %d %d" % (grid, lds, r, row), (ch, bits, spb, streams, got)
    assert lds_of(988) == (996, 63744)  # the headline's rows: 62.25 KiB against the static 129.25 KiB
    # above 2048 coded samples: the scratch path, with an elected recurrence wave while a workgroup has a CU of its own
    got = run(driver, MI355X, ["D %s | 16 16 1 2 4028 1024 1 1 1 1" % K, "D %s | 16 16 1 2 2053 531 1 1 1 1" % K], role)
    assert got == ["split-scratch 0 1024 1 0 %d 4048 %d 0" % (16 * 4048 * 4, r), "split-scratch 0 1024 1 0 %d 2080 %d 0" % (16 * 2080 * 4, r)]
    # past the limits: 4097 recurrences (scratch rows, 257 workgroups) and 8193 (dense)
    got = run(driver, MI355X, ["D %s | 4097 4097 1 4 2016 1024 1 1 1 1" % K, "D %s | 8193 8193 1 4 2016 1024 1 1 1 1" % K,
                               "D 1 0 1 -1 -1 0 | 1000 1000 2 4 992 1024 1 1 1 1"], role)
    assert got == ["split-scratch 0 1024 257 0 %d 2032 0 0" % (4097 * 2032 * 4), "dense 0 64 129 0 0 0 0 0", "dense 1 64 32 0 0 0 0 0"]
    assert run(driver, MI355X, ["D %s | 1000 1000 2 4 992 1024 1 1 1 1" % K], role) == ["split-lds 0 1024 125 63744 0 0 %d 996" % r]  # the headline
