"""Channel-mix window decode on the CPU: the variant list and the launch arithmetic of aad_launch_policy.h
(channel_stream_format_of, channel_mix_variants, plan_channel_mix_window_decode), built with g++ into
tests/channel_mix_policy_driver.cpp; the export of AADHip_ChannelMixWindowDecodePlanCreate; and the numpy statement of the mix
rule (tests/channel_mix_oracle.py) on its corners.

A run is one launch per kernel variant (source channels, bits, mid/side) among the plan's streams, in the fixed order of the six
stereo variants (4-bit L/R, 4-bit M/S, 3-bit L/R, 3-bit M/S, 2-bit L/R, 2-bit M/S), then mono 4-, 3- and 2-bit.  Every launch walks
all N windows with lanes (window, block, SOURCE channel) and is planned as plan_window_decode plans a same-format run of that
variant's channels, bits and smallest block (compared here against tests/window_policy_driver.cpp's output for the same row) - but
for `elements`, which is the output's N * out_channels * T, and whose float32 bytes decide the refusal.  A plan with no variant
(num_streams == 0) plans ONE launch - the mono 4-bit kernel over blocks of T frames - which writes the zeros."""
import os
import subprocess

import numpy as np
import pytest

import aad_amd
from aad_amd.capi import HIP_SYMBOLS
from channel_mix_oracle import channel_mix_expected, mix_stream

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "aad_amd", "csrc")
MI355X = (256, 163840)
SMALL = (32, 65536)
LR, MS = 0, 1
ORDER = [(2, 4, 0), (2, 4, 1), (2, 3, 0), (2, 3, 1), (2, 2, 0), (2, 2, 1), (1, 4, 0), (1, 3, 0), (1, 2, 0)]
SOURCE = {(1, LR): 0, (1, MS): 0, (2, LR): 1, (2, MS): 2}


def _build(tmp, name):
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-I", os.path.join(os.path.dirname(HERE), "include"),
                    "-o", str(exe), os.path.join(HERE, name + ".cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("channel_mix_policy")
    return _build(tmp, "channel_mix_policy_driver"), _build(tmp, "window_policy_driver")


def run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines)
    return out


def fmt(formats):
    """formats: (channels, bits, block_size, samples_per_block, method) per stream"""
    return "%d  %s" % (len(formats), "  ".join("%d %d %d %d %d" % f for f in formats))


def expected_variants(formats):
    """(channels, bits, mid_side, smallest spb, streams) per variant present, in ORDER; mid/side counts for two channels alone"""
    out = []
    for ch, bits, ms in ORDER:
        mine = [f for f in formats if f[0] == ch and f[1] == bits and int(ch == 2 and f[4] == MS) == ms]
        if mine:
            out.append((ch, bits, ms, min(f[3] for f in mine), len(mine)))
    return out


def variants_of(exe, formats):
    got = [int(v) for v in run(exe, ["V %s" % fmt(formats)])[0].split()]
    assert len(got) == 1 + 5 * got[0]
    return [tuple(got[1 + 5 * i:6 + 5 * i]) for i in range(got[0])]


STEREO = [(2, 3, 256, 154, MS), (2, 4, 1024, 992, LR), (2, 2, 128, 188, LR), (2, 4, 256, 224, LR), (2, 3, 1024, 1316, MS),
          (2, 4, 128, 96, MS), (2, 2, 1024, 1980, MS), (2, 4, 1024, 992, LR), (2, 2, 256, 444, LR), (2, 3, 128, 68, LR),
          (2, 4, 256, 224, MS), (2, 4, 128, 96, LR)]
MONO = [(1, 4, 1024, 2012, LR), (1, 2, 128, 444, LR), (1, 3, 256, 634, LR), (1, 4, 128, 220, MS), (1, 3, 128, 292, LR),
        (1, 2, 1024, 4028, MS)]
CORPUS = [f for pair in zip(STEREO, MONO + MONO) for f in pair]  # mono and stereo interleaved


def test_variant_list_dedupe_and_order(drivers):
    exe = drivers[0]
    got = variants_of(exe, CORPUS)
    assert got == expected_variants(CORPUS)
    assert [v[:3] for v in got] == ORDER                                     # all nine, each once, in the fixed order
    assert got[0] == (2, 4, 0, 96, 4) and got[1] == (2, 4, 1, 96, 2)         # smallest spb and stream count per variant
    assert got[6] == (1, 4, 0, 220, 4) and got[8] == (1, 2, 0, 444, 4)
    assert sum(v[4] for v in got) == len(CORPUS)
    # the order does not depend on the streams' order
    assert variants_of(exe, CORPUS[::-1]) == got
    assert variants_of(exe, MONO + STEREO) == variants_of(exe, STEREO + MONO)
    # the stereo variants alone are the mixed-format plan's six; mono alone: three; one format many times: one; none: none
    assert [v[:3] for v in variants_of(exe, STEREO)] == ORDER[:6]
    assert [v[:3] for v in variants_of(exe, MONO)] == ORDER[6:]
    assert variants_of(exe, [STEREO[0]] * 7) == [(2, 3, 1, 154, 7)]
    assert variants_of(exe, [MONO[1]] * 3 + [STEREO[1]]) == [(2, 4, 0, 992, 1), (1, 2, 0, 444, 3)]
    assert variants_of(exe, []) == []


def test_mono_streams_ignore_the_ms_flag(drivers):
    """a mono stream runs the mono kernel whatever its method says (plan create refuses M/S there anyway): the variant key and
    the record's source byte"""
    exe = drivers[0]
    flagged = [f[:4] + (MS,) for f in MONO]
    assert variants_of(exe, flagged) == variants_of(exe, [f[:4] + (LR,) for f in MONO])
    assert all(v[2] == 0 for v in variants_of(exe, flagged))
    rec = [int(v) for v in run(exe, ["R %s" % fmt(CORPUS)])[0].split()]
    assert rec == [v for f in CORPUS for v in (f[3], f[2], f[1], SOURCE[(f[0], f[4])])]
    # a channel count other than 1 or 2 belongs to no variant
    assert variants_of(exe, [(3, 4, 256, 100, LR), (0, 4, 256, 100, LR), (8, 2, 256, 100, LR)]) == []


def touched(phase, frames, spb):
    """blocks whose frames [b spb, (b + 1) spb) meet [phase, phase + frames), counted block by block"""
    b = np.arange(0, (phase + frames) // spb + 3, dtype=np.int64)
    return int(np.count_nonzero((b * spb < phase + frames) & ((b + 1) * spb > phase)))


def parse_plan(line):
    got = [int(v) for v in line.split()]
    ok, count = got[0], got[1]
    assert len(got) == 2 + 10 * count
    return ok, [tuple(got[2 + 10 * i:12 + 10 * i]) for i in range(count)]


@pytest.mark.parametrize("device", [MI355X, SMALL], ids=["mi355x", "32cu_64k"])
@pytest.mark.parametrize("frames", [1, 7, 68, 70, 96, 97, 992, 3000, 48000])
def test_launches_follow_the_source_channels_and_smallest_block_of_each_variant(drivers, device, frames):
    exe, same = drivers
    for out_channels, windows, pad, corpus in ((2, 512, -1, CORPUS), (1, 4096, -1, CORPUS), (2, 100000, -1, MONO), (1, 3, 4096, STEREO),
                                               (1, 0, -1, CORPUS)):
        variants = expected_variants(corpus)
        line = "M %d %d %d %d %d %d %s" % (device + (pad, windows, frames, out_channels, fmt(corpus)))
        ok, launches = parse_plan(run(exe, [line])[0])
        assert ok == 1 and len(launches) == len(variants)
        for (ch, bits, ms, spb, _), launch in zip(variants, launches):
            assert launch[:4] == (ch, bits, ms, spb)
            # K: the brute-force maximum of touched blocks over every phase of that variant's smallest block
            k = max(touched(ph, frames, spb) for ph in range(spb))
            assert launch[4] == k, (frames, spb)
            # lanes: (window, block, SOURCE channel); elements: the OUTPUT's
            assert launch[8] == windows * k * ch and launch[9] == windows * out_channels * frames
            # ... and, but for the elements, the launch plan_window_decode gives a same-format run of those channels, bits and block
            want = run(same, ["W %d %d %d %d %d %d %d %d" % (device + (pad, windows, frames, ch, bits, spb))])[0].split()
            assert want[0] == "1" and [str(v) for v in launch[4:9]] == want[1:6], (frames, out_channels, windows, ch, bits, spb)
            assert int(want[6]) == windows * ch * frames


def test_overflow_is_decided_on_the_outputs_elements(drivers):
    """K <= T and C_source <= 2, so a launch's lanes, N K C_source, never exceed half the float32 bytes of the output,
    4 N out_channels T: the run is refused exactly when those bytes overflow 64 bits - with the OUTPUT's channel count, whatever
    plan_window_decode would say of a run with the source's"""
    exe, same = drivers
    big_s, small_s, big_m, small_m = (2, 4, 1024, 1 << 30, LR), (2, 2, 128, 1, MS), (1, 4, 1024, 1 << 30, LR), (1, 2, 128, 1, LR)
    rows = [  # windows frames out_channels corpus
        (1 << 61, 1, 2, [big_m, small_m]),        # mono sources alone: 2^61 lanes, but 2^64 bytes of output
        (1 << 61, 1, 1, [big_m, small_m]),        # 2^63 bytes: fine
        (1 << 61, 1, 1, [big_s, small_s]),        # stereo sources, 2^62 lanes, 2^63 bytes: fine, though [N, 2, T] would not be
        (1 << 61, 1, 2, [big_s, small_s]),
        (1 << 60, 2, 2, [big_s, big_m]),          # 2^64 bytes
        (1 << 60, 2, 1, [small_s, small_m]),      # 2^63 bytes; lanes 2^62 and 2^61
        (1 << 30, 4294967295, 2, [big_s, small_m]),
        ((1 << 64) - 1, 1, 1, [big_s]),
        (1 << 40, 1 << 20, 2, [big_m, small_m, big_s]),  # 2^63 bytes; K = 2 and 2^20
        ((1 << 40) + 1, 1 << 21, 2, [small_m]),
    ]
    seen = set()
    for windows, frames, out_channels, corpus in rows:
        ok, launches = parse_plan(run(exe, ["M 256 163840 -1 %d %d %d %s" % (windows, frames, out_channels, fmt(corpus))])[0])
        assert ok == int(4 * windows * out_channels * frames < 1 << 64), (windows, frames, out_channels)
        assert len(launches) == (len(expected_variants(corpus)) if ok else 0)  # a refused run plans nothing
        for launch in launches:
            assert launch[8] < 1 << 63 and launch[9] == windows * out_channels * frames
        seen.add(ok)
    assert seen == {0, 1}
    # the two rows whose answer differs from a same-format run with the source's channel count
    assert run(same, ["W 256 163840 -1 %d 1 1 4 %d" % (1 << 61, 1 << 30)])[0].split()[0] == "1"
    assert run(same, ["W 256 163840 -1 %d 1 2 4 %d" % (1 << 61, 1 << 30)])[0].split()[0] == "0"
    ok, launches = parse_plan(run(exe, ["M 256 163840 -1 %d %d 2 %s" % (1 << 40, 1 << 20, fmt([big_m, small_m, big_s]))])[0])
    assert [l[4] for l in launches] == [2, 2, 1 << 20] and [l[8] for l in launches] == [1 << 42, 1 << 41, 1 << 60]
    # T = 0 and an output channel count outside {1, 2}
    assert parse_plan(run(exe, ["M 256 163840 -1 1 0 2 %s" % fmt([big_s])])[0]) == (0, [])
    assert parse_plan(run(exe, ["M 256 163840 -1 1 100 0 %s" % fmt([big_s])])[0]) == (0, [])
    assert parse_plan(run(exe, ["M 256 163840 -1 1 100 3 %s" % fmt([big_s])])[0]) == (0, [])


def test_no_streams_plans_one_zero_writing_launch(drivers):
    """num_streams == 0: no variant, and ONE launch - the mono 4-bit kernel over blocks of T frames, K = 2 (1 for T = 1) - whose
    lanes all find their window's stream out of range and write its zeros into out_channels rows each"""
    exe, same = drivers
    for frames in (1, 2, 3000):
        for out_channels in (1, 2):
            ok, launches = parse_plan(run(exe, ["M 256 163840 -1 512 %d %d 0" % (frames, out_channels)])[0])
            assert ok == 1 and len(launches) == 1
            k = 1 if frames == 1 else 2
            assert launches[0][:5] == (1, 4, 0, frames, k)
            want = run(same, ["W 256 163840 -1 512 %d 1 4 %d" % (frames, frames)])[0].split()
            assert [str(v) for v in launches[0][4:9]] == want[1:6]
            assert launches[0][8] == 512 * k and launches[0][9] == 512 * out_channels * frames


def test_library_exports_the_constructor():
    lib = aad_amd.load_library()
    assert "AADHip_ChannelMixWindowDecodePlanCreate" in HIP_SYMBOLS
    assert hasattr(lib, "AADHip_ChannelMixWindowDecodePlanCreate")
    text = open(os.path.join(os.path.dirname(HERE), "include", "aad_hip.h")).read()
    assert "AADHip_ChannelMixWindowDecodePlanCreate(" in text


# ---- the numpy statement of the mix rule ---------------------------------------------------------------------------------------
CORNERS = [(-32768, -32768), (-2, -1), (-1, -2), (-3, 0), (-1, 0), (0, -1), (0, 0), (1, 0), (0, 1), (32767, 32767), (32767, -32768),
           (-32768, 32767), (5, -8), (-32768, 32765)]


def test_oracle_down_mix_corners():
    d = np.array(CORNERS, dtype=np.int16)
    sums = [l + r for l, r in CORNERS]
    assert {-65536, -3, -1, 0, 1, 65534} <= set(sums)
    got16 = mix_stream(d, 1, np.int16)
    got32 = mix_stream(d, 1, np.float32)
    assert got16.dtype == np.int16 and got32.dtype == np.float32 and got16.shape == got32.shape == (len(CORNERS), 1)
    for i, s in enumerate(sums):
        assert int(got16[i, 0]) == s // 2                      # the floor, not truncation
        want = np.float32(s) / np.float32(65536)
        assert got32[i, 0].view(np.uint32) == want.view(np.uint32)
        assert float(got32[i, 0]) == s / 65536.0               # exact: the half step is kept
    by_sum = {s: int(got16[i, 0]) for i, s in enumerate(sums)}
    assert by_sum[-65536] == -32768 and by_sum[-3] == -2 and by_sum[-1] == -1 and by_sum[1] == 0 and by_sum[65534] == 32767
    # float32 is not the int16 mix / 32768 where the sum is odd
    odd = [i for i, s in enumerate(sums) if s % 2]
    assert odd and all(float(got32[i, 0]) != float(got16[i, 0]) / 32768.0 for i in odd)


def test_oracle_same_count_twin_rows_and_windows():
    mono = np.array([[-32768], [7], [32767], [-1]], dtype=np.int16)
    stereo = np.array(CORNERS, dtype=np.int16)
    assert np.array_equal(mix_stream(mono, 1), mono) and np.array_equal(mix_stream(stereo, 2), stereo)
    assert np.array_equal(mix_stream(mono, 2), np.repeat(mono, 2, axis=1))
    assert np.array_equal(mix_stream(mono, 2, np.float32), np.repeat(mono, 2, axis=1).astype(np.float32) / np.float32(32768))
    assert np.array_equal(mix_stream(stereo, 2, np.float32), stereo.astype(np.float32) / np.float32(32768))
    windows = [(0, 1), (1, 12), (1, len(CORNERS)), (2, 0), (-1, 0), (0, -1), (0, 1 << 40)]
    for out_channels in (1, 2):
        for dtype in (np.int16, np.float32):
            got = channel_mix_expected([mono, stereo], windows, 5, out_channels, dtype)
            assert got.shape == (len(windows), out_channels, 5) and got.dtype == dtype
            assert np.array_equal(got[0, :, :3], mix_stream(mono, out_channels, dtype)[1:].T) and not got[0, :, 3:].any()
            assert np.array_equal(got[1, :, :2], mix_stream(stereo, out_channels, dtype)[12:].T) and not got[1, :, 2:].any()
            assert not got[2:].any()  # at the end, stream out of range, wrapped, huge
