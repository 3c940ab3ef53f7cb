"""Mixed-format window decode on the CPU: the variant list and the launch arithmetic of aad_launch_policy.h (stream_format_of,
window_variants, plan_mixed_window_decode), built with g++ into tests/mixed_window_policy_driver.cpp, and the export of
AADHip_MixedWindowDecodePlanCreate.

A run is one launch per kernel variant (bits, mid/side) among the plan's streams, in the fixed order 4-bit L/R, 4-bit M/S, 3-bit
L/R, 3-bit M/S, 2-bit L/R, 2-bit M/S.  Every launch walks all N windows with K = window_blocks_spanned(T, the smallest
samples_per_block among that variant's streams) blocks per window and is otherwise planned as plan_window_decode plans a
same-format run of that variant's bits (compared here against tests/window_policy_driver.cpp's output for the same row).  A plan
with no variant (num_streams == 0) plans ONE launch - the 4-bit L/R kernel over blocks of T frames - which writes the zeros."""
import os
import subprocess

import numpy as np
import pytest

import aad_amd
from aad_amd.capi import HIP_SYMBOLS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "aad_amd", "csrc")
MI355X = (256, 163840)
SMALL = (32, 65536)
LR, MS = 0, 1
ORDER = [(4, 0), (4, 1), (3, 0), (3, 1), (2, 0), (2, 1)]


def _build(tmp, name):
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-I", os.path.join(os.path.dirname(HERE), "include"),
                    "-o", str(exe), os.path.join(HERE, name + ".cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mixed_window_policy")
    return _build(tmp, "mixed_window_policy_driver"), _build(tmp, "window_policy_driver")


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


def fmt(formats):
    """formats: (bits, block_size, samples_per_block, method) per stream"""
    return "%d  %s" % (len(formats), "  ".join("%d %d %d %d" % f for f in formats))


def expected_variants(channels, formats):
    """(bits, mid_side, smallest spb, streams) per variant present, in ORDER; mid/side counts for two channels alone"""
    out = []
    for bits, ms in ORDER:
        mine = [f for f in formats if f[0] == bits and int(channels == 2 and f[3] == MS) == ms]
        if mine:
            out.append((bits, ms, min(f[2] for f in mine), len(mine)))
    return out


def variants_of(exe, channels, formats):
    got = [int(v) for v in run(exe, ["V %d %s" % (channels, fmt(formats))])[0].split()]
    assert len(got) == 1 + 4 * got[0]
    return [tuple(got[1 + 4 * i:5 + 4 * i]) for i in range(got[0])]


STEREO = [(3, 256, 154, MS), (4, 1024, 992, LR), (2, 128, 188, LR), (4, 256, 224, LR), (3, 1024, 1316, MS), (4, 128, 96, MS),
          (2, 1024, 1980, MS), (4, 1024, 992, LR), (2, 256, 444, LR), (3, 128, 68, LR), (4, 256, 224, MS), (4, 128, 96, LR)]


def test_variant_list_dedupe_and_order(drivers):
    exe = drivers[0]
    got = variants_of(exe, 2, STEREO)
    assert got == expected_variants(2, STEREO)
    assert [(b, m) for b, m, _, _ in got] == ORDER                      # all six, each once, in the fixed order
    assert got[0] == (4, 0, 96, 4) and got[1] == (4, 1, 96, 2)          # smallest spb and stream count per variant
    # the order does not depend on the streams' order
    assert variants_of(exe, 2, STEREO[::-1]) == got
    # stereo without M/S: three variants; one format many times: one
    lr = [f for f in STEREO if f[3] == LR]
    assert [(b, m) for b, m, _, _ in variants_of(exe, 2, lr)] == [(4, 0), (3, 0), (2, 0)]
    assert variants_of(exe, 2, [STEREO[0]] * 7) == [(3, 1, 154, 7)]
    assert variants_of(exe, 2, []) == []


@pytest.mark.parametrize("channels", [1, 3, 8])
def test_other_channel_counts_ignore_the_ms_flag(drivers, channels):
    """launch_decode_window takes the M/S instantiation for `channels == 2 && mid_side` alone; so does the variant key and the
    record's mid_side byte (plan create refuses M/S on other channel counts anyway)"""
    exe = drivers[0]
    got = variants_of(exe, channels, STEREO)
    assert got == expected_variants(channels, STEREO)
    assert [(b, m) for b, m, _, _ in got] == [(4, 0), (3, 0), (2, 0)]
    assert sum(v[3] for v in got) == len(STEREO)
    rec = [int(v) for v in run(exe, ["R %d %s" % (channels, fmt(STEREO))])[0].split()]
    assert rec == [v for f in STEREO for v in (f[2], f[1], f[0], 0)]
    rec2 = [int(v) for v in run(exe, ["R 2 %s" % fmt(STEREO)])[0].split()]
    assert rec2 == [v for f in STEREO for v in (f[2], f[1], f[0], f[3])]


def touched(phase, frames, spb):
    """blocks whose frames [b spb, (b + 1) spb) meet [phase, phase + frames), counted block by block"""
    b = np.arange(0, (phase + frames) // spb + 3, dtype=np.int64)
    return int(np.count_nonzero((b * spb < phase + frames) & ((b + 1) * spb > phase)))


def parse_plan(line):
    got = [int(v) for v in line.split()]
    ok, count = got[0], got[1]
    assert len(got) == 2 + 9 * count
    return ok, [tuple(got[2 + 9 * i:11 + 9 * i]) for i in range(count)]


@pytest.mark.parametrize("device", [MI355X, SMALL], ids=["mi355x", "32cu_64k"])
@pytest.mark.parametrize("frames", [1, 7, 68, 70, 96, 97, 992, 3000, 48000])
def test_launches_follow_the_smallest_block_of_each_variant(drivers, device, frames):
    exe, same = drivers
    for channels, windows, pad in ((2, 512, -1), (1, 4096, -1), (2, 100000, -1), (8, 3, 4096), (2, 0, -1)):
        variants = expected_variants(channels, STEREO)
        ok, launches = parse_plan(run(exe, ["M %d %d %d %d %d %d %s" % (device + (pad, windows, frames, channels, fmt(STEREO)))])[0])
        assert ok == 1 and len(launches) == len(variants)
        for (bits, ms, spb, _), launch in zip(variants, launches):
            assert launch[:3] == (bits, ms, spb)
            # K: the brute-force maximum of touched blocks over every phase of that variant's smallest block
            assert launch[3] == max(touched(ph, frames, spb) for ph in range(spb)), (frames, spb)
            # ... and the launch that plan_window_decode gives a same-format run of those bits and that block
            want = run(same, ["W %d %d %d %d %d %d %d %d" % (device + (pad, windows, frames, channels, bits, spb))])[0]
            assert "1 %d %d %d %d %d %d" % launch[3:] == want, (frames, channels, windows, bits, spb)
            # a stream of the variant with longer blocks needs no more lanes per window than K
            for f in STEREO:
                if f[0] == bits and int(channels == 2 and f[3] == MS) == ms:
                    assert max(touched(ph, frames, f[2]) for ph in (0, f[2] - 1)) <= launch[3]


def test_overflow_refused_if_any_launch_overflows(drivers):
    """the run is refused exactly when plan_window_decode refuses one of its launches (K <= T, so a launch's lanes never exceed the
    output's elements: what overflows first is the elements' float32 bytes, the same for every launch)"""
    exe, same = drivers
    big, small = (4, 1024, 1 << 30, LR), (2, 128, 1, LR)
    rows = [  # windows frames channels
        (1 << 61, 2, 1),             # 2^62 elements: 2^64 float32 bytes
        (1 << 62, 2, 2),             # 2^64 elements
        (1 << 30, 4294967295, 8),    # lanes and elements past 2^64
        ((1 << 64) - 1, 1, 8),
        (1 << 60, 1, 1),             # 2^62 bytes: fine
        (1 << 40, 1 << 20, 1),       # 2^62 bytes; K = 2 and K = 2^20
        (1 << 42, (1 << 20) + 1, 3),
    ]
    seen = set()
    for windows, frames, channels in rows:
        per = [run(same, ["W 256 163840 -1 %d %d %d %d %d" % (windows, frames, channels, f[0], f[2])])[0].split()[0] for f in (big, small)]
        ok, launches = parse_plan(run(exe, ["M 256 163840 -1 %d %d %d %s" % (windows, frames, channels, fmt([big, small]))])[0])
        assert ok == int(per == ["1", "1"]), (windows, frames, channels, per)
        assert len(launches) == (2 if ok else 0)  # a refused run plans nothing
        seen.add(ok)
    assert seen == {0, 1}
    ok, launches = parse_plan(run(exe, ["M 256 163840 -1 %d %d 1 %s" % (1 << 40, 1 << 20, fmt([big, small]))])[0])
    assert [l[3] for l in launches] == [2, 1 << 20] and [l[7] for l in launches] == [1 << 41, 1 << 60]
    assert parse_plan(run(exe, ["M 256 163840 -1 1 0 2 %s" % fmt([big])])[0]) == (0, [])  # T = 0


def test_no_streams_plans_one_zero_writing_launch(drivers):
    """num_streams == 0: no variant, and ONE launch - the 4-bit L/R kernel over blocks of T frames, K = 2 (1 for T = 1) - whose
    lanes all find their window's stream out of range and write its zeros"""
    exe, same = drivers
    for frames in (1, 2, 3000):
        for channels in (1, 2, 8):
            ok, launches = parse_plan(run(exe, ["M 256 163840 -1 512 %d %d 0" % (frames, channels)])[0])
            assert ok == 1 and len(launches) == 1
            assert launches[0][:4] == (4, 0, frames, 1 if frames == 1 else 2)
            assert "1 %d %d %d %d %d %d" % launches[0][3:] == run(same, ["W 256 163840 -1 512 %d %d 4 %d" % (frames, channels, frames)])[0]
            assert launches[0][7] == 512 * channels * launches[0][3]


def test_library_exports_the_constructor():
    lib = aad_amd.load_library()
    assert "AADHip_MixedWindowDecodePlanCreate" in HIP_SYMBOLS
    assert hasattr(lib, "AADHip_MixedWindowDecodePlanCreate")
    text = open(os.path.join(os.path.dirname(HERE), "include", "aad_hip.h")).read()
    assert "AADHip_MixedWindowDecodePlanCreate(" in text
