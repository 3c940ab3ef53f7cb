"""aad_amd/csrc/aad_fir_stage.h, the one rule of what a Resolve and a Run of the FIR stages (resample, convolve) refuse, built with g++
into tests/fir_stage_driver.cpp.  Every expected value below is written out from the arithmetic: a run is refused when one of
rows = windows * channels, rows * frames * elem, rows * source_frames * 2 and rows * tiles reaches 2^64."""
import os
import subprocess

import pytest

from aad_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "aad_amd", "csrc")
RESAMPLE_TILE, CONVOLVE_TILE = 1024, 4096  # kResampleTile: 256 threads x 4 outputs; kConvolveTile: 4 waves x 4 blocks x 256 outputs
SRC, LANES, OUT = 0x1000, 0x2000, 0x3000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fir_stage") / "fir_stage_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "fir_stage_driver.cpp")],
                   check=True)
    return str(exe)


def _ask(driver, lines):
    out = subprocess.run([driver], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines)
    return out


def rows(windows=2, channels=1, frames=8, source_frames=8, needed=8, elem=4, src=SRC, lanes=LANES, out=OUT, out_optional=0,
         tile=RESAMPLE_TILE):
    return "rows %d %d %d %d %d %d %d %d %d %d %d" % (windows, channels, frames, source_frames, needed, elem, src, lanes, out, out_optional, tile)


def test_tiles_at_both_stages_tile_sizes(driver):
    assert _ask(driver, ["tiles"]) == ["%d %d" % (RESAMPLE_TILE, CONVOLVE_TILE)]
    for tile in (RESAMPLE_TILE, CONVOLVE_TILE):
        cases = ((1, 1), (tile, 1), (tile + 1, 2))
        got = _ask(driver, [rows(windows=3, channels=2, frames=t, source_frames=t, needed=t, tile=tile) for t, _ in cases])
        assert got == ["ok 6 %d" % tiles for _, tiles in cases]


def test_each_product_at_the_last_operands_that_fit_and_the_first_that_do_not(driver):
    """One product at a time, every other one kept below 2^64 where the arithmetic allows it.  rows * tiles <= rows * frames and
    rows < rows * frames * elem, so neither the row count nor the item count can be the ONLY product past 64 bits with honest
    operands: the row count is shown by 2^63 windows x 2 channels, whose product wraps to 0 rows and so passes every later
    product, and at its largest value that fits, (2^32 + 1)(2^32 - 1) = 2^64 - 1, which the bytes then refuse; the item count at
    the largest value a run can give it, 2^63 - 1 rows of one tile."""
    cases = [
        # rows * frames * elem: 2^31 * 2^31 * 2 = 2^63 fits, * 4 = 2^64 does not (the source rows: 1 frame, 2^32 bytes)
        (rows(windows=1 << 31, frames=1 << 31, source_frames=1, needed=1, elem=2), "ok %d %d" % (1 << 31, (1 << 31) // RESAMPLE_TILE)),
        (rows(windows=1 << 31, frames=1 << 31, source_frames=1, needed=1, elem=4), "refused"),
        (rows(windows=1 << 31, frames=1 << 31, source_frames=1, needed=1, elem=2, tile=CONVOLVE_TILE), "ok %d %d" % (1 << 31, (1 << 31) // CONVOLVE_TILE)),
        # ... to the element: 2 frames of 1 source frame, so that the source's bytes stay at half the rows'
        (rows(windows=(1 << 62) - 1, frames=2, source_frames=1, needed=1, elem=2), "ok %d 1" % ((1 << 62) - 1)),  # 2^64 - 4 bytes
        (rows(windows=1 << 62, frames=2, source_frames=1, needed=1, elem=2), "refused"),                          # 2^64
        (rows(windows=(1 << 62) - 1, frames=1, source_frames=1, needed=1, elem=4), "ok %d 1" % ((1 << 62) - 1)),
        (rows(windows=1 << 62, frames=1, source_frames=1, needed=1, elem=4), "refused"),
        # rows * source_frames * 2, the rows' bytes at 2^63 or below: elem 2 with 1 frame of 2 source frames, elem 4 of 4
        (rows(windows=(1 << 62) - 1, frames=1, source_frames=2, needed=2, elem=2), "ok %d 1" % ((1 << 62) - 1)),
        (rows(windows=1 << 62, frames=1, source_frames=2, needed=2, elem=2), "refused"),
        (rows(windows=(1 << 61) - 1, frames=1, source_frames=4, needed=4, elem=4), "ok %d 1" % ((1 << 61) - 1)),
        (rows(windows=1 << 61, frames=1, source_frames=4, needed=4, elem=4), "refused"),
        # windows * channels: 2^64 wraps to 0 rows; 2^64 - 1 rows fit and their bytes do not; both element sizes
        (rows(windows=1 << 63, channels=2, frames=1, source_frames=1, needed=1, elem=2), "refused"),
        (rows(windows=1 << 63, channels=2, frames=1, source_frames=1, needed=1, elem=4), "refused"),
        (rows(windows=(1 << 32) + 1, channels=(1 << 32) - 1, frames=1, source_frames=1, needed=1, elem=2), "refused"),
        (rows(windows=1 << 31, channels=(1 << 32) - 1, frames=1, source_frames=1, needed=1, elem=2), "ok %d 1" % ((1 << 31) * ((1 << 32) - 1))),
        # rows * tiles: one tile a row, at the most rows whose bytes fit - 2^63 - 1 of elem 2, 2^62 - 1 of elem 4 (above)
        (rows(windows=(1 << 63) - 1, frames=1, source_frames=1, needed=1, elem=2), "ok %d 1" % ((1 << 63) - 1)),
        (rows(windows=1 << 63, frames=1, source_frames=1, needed=1, elem=2), "refused"),
        # ... and with more tiles than one: 2^32 - 1 frames are 2^22 tiles of 1024, rows * frames * elem at 2^64 - 2^32 and past it
        (rows(windows=1 << 31, frames=(1 << 32) - 1, source_frames=1, needed=1, elem=2), "ok %d %d" % (1 << 31, 1 << 22)),
        (rows(windows=(1 << 31) + 1, frames=(1 << 32) - 1, source_frames=1, needed=1, elem=2), "refused"),
    ]
    assert _ask(driver, [c for c, _ in cases]) == [want for _, want in cases]


def test_alignment_nulls_and_source_length(driver):
    cases = [
        (rows(), "ok 2 1"),
        # out: a multiple of the element - bit 1 set is aligned for 2 bytes and not for 4; bit 0 for neither
        (rows(elem=2, out=OUT + 2), "ok 2 1"), (rows(elem=4, out=OUT + 2), "refused"), (rows(elem=2, out=OUT + 1), "refused"),
        (rows(src=SRC + 1), "refused"), (rows(src=SRC + 2), "ok 2 1"),
        (rows(lanes=LANES + 2), "refused"), (rows(lanes=LANES + 1), "refused"), (rows(lanes=LANES + 4), "ok 2 1"),
        (rows(source_frames=8, needed=8), "ok 2 1"), (rows(source_frames=7, needed=8), "refused"), (rows(source_frames=9, needed=8), "ok 2 1"),
        (rows(src=0), "refused"), (rows(lanes=0), "refused"),
        (rows(out=0), "refused"), (rows(out=0, out_optional=1), "ok 2 1"), (rows(out_optional=1), "ok 2 1"),
        (rows(channels=0), "refused"), (rows(frames=0, source_frames=0, needed=0), "refused"), (rows(windows=0), "ok 0 1"),
    ]
    assert _ask(driver, [c for c, _ in cases]) == [want for _, want in cases]


def test_resolve_rule(driver):
    most = (2 ** 31 - 1) * 256  # INT32_MAX blocks of 256 windows
    cases = [
        ("resolve %d 4096 8192 12288 16384" % most, "ok"), ("resolve %d 4096 8192 12288 16384" % (most + 1), "refused"),
        ("resolve 2 4096 0 12288 16384", "ok"),  # the selector alone may be null
        ("resolve 2 0 8192 12288 16384", "refused"), ("resolve 2 4096 8192 0 16384", "refused"), ("resolve 2 4096 8192 12288 0", "refused"),
        ("resolve 2 4100 8192 12288 16384", "refused"), ("resolve 2 4096 8196 12288 16384", "refused"),
        ("resolve 2 4096 8192 12292 16384", "refused"), ("resolve 2 4096 8192 12288 16388", "ok"), ("resolve 2 4096 8192 12288 16386", "refused"),
    ]
    assert _ask(driver, [c for c, _ in cases]) == [want for _, want in cases]


def test_gain_rule(driver):
    store, add = capi.WINDOW_GAIN_STORE, capi.WINDOW_GAIN_ADD
    assert (capi.SAMPLE_INT16, store, add) == (0, 0, 1)
    cases = [("gain %d %d 4096 8192" % (t, m), "ok") for t in (capi.SAMPLE_FLOAT32, capi.SAMPLE_FLOAT16, capi.SAMPLE_BFLOAT16)
             for m in (store, add)]
    cases += [
        ("gain %d %d 4096 8192" % (capi.SAMPLE_INT16, store), "refused"), ("gain %d 2 4096 8192" % capi.SAMPLE_FLOAT32, "refused"),
        ("gain %d -1 4096 8192" % capi.SAMPLE_FLOAT32, "refused"),
        ("gain %d %d 4098 8192" % (capi.SAMPLE_FLOAT32, store), "refused"), ("gain %d %d 4100 8192" % (capi.SAMPLE_FLOAT32, store), "ok"),
        ("gain %d %d 4096 8196" % (capi.SAMPLE_FLOAT32, store), "refused"),
        ("gain %d %d 0 0" % (capi.SAMPLE_FLOAT32, add), "ok"),  # either table may be null
    ]
    assert _ask(driver, [c for c, _ in cases]) == [want for _, want in cases]
