"""The chain table of a segmented encode plan (aad_amd/csrc/aad_segments.h), on the CPU: tests/segment_plan_driver.cpp is built
with g++ against the header and prints the table of every batch.  The expected rows are worked out by hand from the definition in
include/aad_hip.h: segment s keeps blocks [s L, min((s + 1) L, B)) and its chain encodes frames [(s L - w) spb, min((s + 1) L spb,
N)), w = min(W, s L).

Row: pcm_offset data_offset first_block num_frames warmup_blocks header_samples writes_header."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "aad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("segments") / "segment_plan_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "segment_plan_driver.cpp")], check=True)
    return str(exe)


def table(driver, channels, spb, block_size, L, W, streams):
    """streams: [(pcm_offset, data_offset, num_samples)] -> ("ok" | "refused", count, [row tuples])"""
    lines = ["%d %d %d %d %d %d" % (channels, spb, block_size, L, W, len(streams))]
    lines += ["%d %d %d" % s for s in streams]
    out = subprocess.run([driver], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    status, count = out[0].split()
    rows = [tuple(int(v) for v in r.split()) for r in out[1:] if r.strip()]
    return status, int(count), rows


def test_one_chain_when_the_segment_covers_the_stream(driver):
    for L in (10, 11, 1000, 0xFFFFFFFF):
        assert table(driver, 2, 10, 40, L, 4, [(1000, 64, 95)]) == ("ok", 1, [(1000, 64, 0, 95, 0, 95, 1)])


def test_warmup_clamped_at_the_start_and_short_last_block(driver):
    # B = 10 blocks, the last one 5 frames; L = 3, W = 5: segment 1 can only warm up over blocks 0..2
    assert table(driver, 2, 10, 40, 3, 5, [(1000, 64, 95)]) == ("ok", 4, [
        (1000, 64, 0, 30, 0, 95, 1),
        (1000, 64, 0, 60, 3, 95, 0),
        (1020, 64, 1, 80, 5, 95, 0),
        (1080, 64, 4, 55, 5, 95, 0),
    ])


def test_streams_of_one_frame_and_shorter_than_a_block(driver):
    assert table(driver, 1, 10, 40, 1, 3, [(0, 0, 1), (1, 100, 7), (8, 200, 10), (18, 300, 11)]) == ("ok", 5, [
        (0, 0, 0, 1, 0, 1, 1),
        (1, 100, 0, 7, 0, 7, 1),
        (8, 200, 0, 10, 0, 10, 1),
        (18, 300, 0, 10, 0, 11, 1),
        (18, 300, 0, 11, 1, 11, 0),
    ])


def test_blocks_an_exact_multiple_of_the_segment(driver):
    assert table(driver, 2, 10, 40, 5, 2, [(0, 0, 100)]) == ("ok", 2, [
        (0, 0, 0, 50, 0, 100, 1),
        (60, 0, 3, 70, 2, 100, 0),
    ])
    # no warm-up: the segments tile the stream
    assert table(driver, 2, 10, 40, 5, 0, [(0, 0, 100)]) == ("ok", 2, [
        (0, 0, 0, 50, 0, 100, 1),
        (100, 0, 5, 50, 0, 100, 0),
    ])


def test_eight_channels(driver):
    assert table(driver, 8, 10, 200, 2, 1, [(64, 4096, 50)]) == ("ok", 3, [
        (64, 4096, 0, 20, 0, 50, 1),
        (144, 4096, 1, 30, 1, 50, 0),
        (304, 4096, 3, 20, 1, 50, 0),
    ])


def test_offsets_beyond_32_bits(driver):
    # 4e9 frames of 8 channels, four samples per block: frame and byte offsets far past 2^32
    n, L, W = 4000000000, 1 << 29, 8
    pcm0, data0 = 3 << 32, (5 << 32) + 7
    status, count, rows = table(driver, 8, 4, 36, L, W, [(pcm0, data0, n)])
    first = (L - W) * 4
    assert (status, count) == ("ok", 2)
    assert rows == [(pcm0, data0, 0, L * 4, 0, n, 1), (pcm0 + first * 8, data0, L - W, n - first, W, n, 0)]


def test_refusals(driver):
    # more than UINT32_MAX chains: four streams of 2^30 blocks, one block per chain, is exactly 2^32 chains
    big = [(0, 0, 0xFFFFFFFF)] * 4
    assert table(driver, 1, 4, 20, 1, 0, big) == ("refused", 1 << 32, [])
    assert table(driver, 1, 4, 20, 1, 0, big * 2) == ("refused", 1 << 33, [])
    assert table(driver, 1, 10, 40, 0, 0, [(0, 0, 100)]) == ("refused", 0, [])
