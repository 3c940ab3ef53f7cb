"""Window reconstruct on the CPU (include/aad_hip.h "window reconstruct"): the library exports the three entry points; the
arithmetic the resolve kernel runs on the device (aad_amd/csrc/aad_windows.h, compiled here with g++ through
tests/window_reconstruct_host_driver.cpp) gives the window lengths of the definition and, lane for lane, the records the host
builders of aad_segments.h give for the crop as a stream of its own; and the run's refusals (image stride, overlapping rows,
64-bit overflow, lane count, source rows)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
I16, F32 = 0, 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("window_reconstruct") / "window_reconstruct_host_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o",
                    str(exe), os.path.join(ROOT, "tests", "window_reconstruct_host_driver.cpp")], check=True)
    return str(exe)


def test_library_exports_the_three_entry_points():
    from aad_amd.capi import HIP_SYMBOLS, load_library
    lib = load_library()
    for name in ("AADHip_WindowReconstructPlanCreate", "AADHip_WindowReconstructPlanRun", "AADHip_WindowReconstructPlanDestroy"):
        assert name in HIP_SYMBOLS
        getattr(lib, name)


def window_length(sources, stream, first, frames):
    """the definition, written out"""
    if stream >= len(sources) or first >= sources[stream]:
        return 0
    return min(frames, sources[stream] - first)


def test_lengths_and_lanes_follow_the_definition_and_the_host_builders(driver):
    cases = []
    for spb in (64, 100):
        sources = [1, 37, spb, 3 * spb + 5, 5 * spb + 77, 0]
        for frames in (1, spb - 1, spb, 3 * spb + 11, 8 * spb):
            for L, W in ((0, 0), (1, 0), (1, 3), (2, 1), (3, 3), (8, 2), (1000, 5)):
                for s, n in enumerate(sources):
                    firsts = {0, 1, spb // 2, spb, spb + 7, max(n - 1, 0), n, n + 1, max(n - frames, 0), max(n - frames + 1, 0),
                              1 << 63, (1 << 64) - 1}
                    for first in sorted(firsts):
                        cases.append((spb, L, W, frames, sources, s, first))
                for s in (len(sources), len(sources) + 1, 1 << 63, (1 << 64) - 1):  # a stream index of S and beyond
                    cases.append((spb, L, W, frames, sources, s, 0))
    lines = []
    for i, (spb, L, W, frames, sources, s, first) in enumerate(cases):
        w = (0, 1, 5, 4000)[i % 4]
        lines.append("%d %d %d %d %d %d %d %d %d %d %d %s" % (spb, L, W, frames, 4096 + 64 * (i % 3), 2 * frames + i % 5, 7 + i % 11, w,
                                                               len(sources), s, first, " ".join(str(v) for v in sources)))
    out = subprocess.run([driver, "lanes"], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases) > 4000
    seen_padding = seen_partial = False
    for (spb, L, W, frames, sources, s, first), line in zip(cases, out):
        got_len, per, real, verdict = line.split(" ", 3)
        want = window_length(sources, s, first, frames)
        assert int(got_len) == want, (spb, L, W, frames, s, first, line)
        full = -(-frames // spb)
        assert int(per) == (1 if L == 0 else max(1, -(-full // L))), line
        blocks = -(-want // spb)
        assert int(real) == (1 if L == 0 else max(1, -(-blocks // L))), line
        assert verdict == "same", (spb, L, W, frames, s, first, line)
        seen_padding |= int(real) < int(per)
        seen_partial |= 0 < want < frames
    assert seen_padding and seen_partial


def verdicts(driver, lines):
    out = subprocess.run([driver, "refuse"], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(lines)
    return out


def test_refuses_a_short_image_stride_and_images_past_64_bits(driver):
    assert verdicts(driver, ["images 2 1054 1055", "images 4096 0 1055", "images 3 %d 1055" % (1 << 63),
                             "images 2 %d 100" % ((1 << 64) - 50)]) == ["refused"] * 4
    assert verdicts(driver, ["images 2 1055 1055", "images 1 0 1055", "images 0 0 1055", "images 4096 1088 1055",
                             "images 2 %d 100" % ((1 << 64) - 101)]) == ["ok"] * 5


def test_refuses_overlapping_rows_and_row_overflow(driver):
    big = 1 << 63
    refused = ["rows 2 4 100 %d 0 200 99" % I16,          # channel rows of T elements overlap
               "rows 2 4 100 %d 0 199 100" % F32,         # window w's last row runs into window w + 1's first
               "rows 1 2 100 %d 0 99 0" % I16,            # mono rows overlap
               "rows 2 4 100 2 0 200 100",                # unknown sample type
               "rows 2 4 100 %d 1 200 100" % F32,         # reserved
               "rows 2 1 100 %d 0 200 %d" % (I16, big),   # (C - 1) cs + T: fits in elements, not in bytes
               "rows 2 3 100 %d 0 %d 100" % (I16, big),   # (N - 1) ss overflows
               "rows 2 2 100 %d 0 %d 100" % (F32, (1 << 62) - 1),  # element offsets fit, float32 bytes do not
               "rows 1 %d 100 %d 0 %d 0" % (1 << 33, I16, 1 << 31)]  # 2^33 windows 2^31 elements apart
    assert verdicts(driver, refused) == ["refused"] * len(refused)
    ok = ["rows 2 4 100 %d 0 200 100" % F32, "rows 1 1 100 %d 0 0 0" % I16, "rows 3 0 100 %d 0 5 100" % I16,
          "rows 2 2 100 %d 0 %d 100" % (I16, 1 << 62)]
    assert verdicts(driver, ok) == ["ok"] * len(ok)


def test_refuses_more_lanes_than_32_bits(driver):
    # 49 blocks of 992 frames: 49 lanes per window at L = 1, 7 at L = 8, one unsegmented
    assert verdicts(driver, ["lanes %d 48000 992 0" % ((1 << 32) - 1), "lanes %d 48000 992 1" % (((1 << 32) - 1) // 49),
                             "lanes %d 48000 992 8" % (((1 << 32) - 1) // 7), "lanes 0 48000 992 1"]) == ["ok"] * 4
    assert verdicts(driver, ["lanes %d 48000 992 0" % (1 << 32), "lanes %d 48000 992 1" % (((1 << 32) - 1) // 49 + 1),
                             "lanes %d 48000 992 8" % (((1 << 32) - 1) // 7 + 1), "lanes %d 48000 992 1" % ((1 << 64) - 1),
                             "lanes 5 48000 0 1"]) == ["refused"] * 5


def test_refuses_source_rows_that_overlap_or_overflow(driver):
    big = 1 << 63
    assert verdicts(driver, ["sources 2 99 2 2 0 50 1000 100",              # channel_stride below the longest stream
                             "sources 2 %d 2 1 0 100" % big,                # fits in elements, not in int16 bytes
                             "sources 3 %d 2 1 0 100" % big,                # (C - 1) cs overflows
                             "sources 1 0 4 1 %d 100" % ((1 << 62) - 50),   # float32 bytes overflow
                             "sources 1 0 2 1 %d 100" % ((1 << 64) - 50)]) == ["refused"] * 5
    assert verdicts(driver, ["sources 2 100 2 3 1 100 301 0 777 37", "sources 1 0 4 2 5 100 3 100", "sources 2 5 2 0",
                             "sources 1 0 2 1 %d 100" % ((1 << 63) - 101)]) == ["ok"] * 4
