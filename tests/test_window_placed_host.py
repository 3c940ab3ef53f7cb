"""Window decode with a span per window (AADHip_WindowDecodePlanRunPlaced / ...RunPlacedStats), what can be checked without a device:
  * the symbols: in include/aad_hip.h and in HIP_SYMBOLS with argtypes, the 16-byte struct;
  * tests/window_placed_oracle.py pinned on hand-computed cases;
  * aad_amd/csrc/aad_window_span.h - the clip, the crop range and the fill tile the kernels run - built with g++ into
    tests/window_span_driver.cpp and held against a brute force over every element of the row;
  * the engine's refusals and routing, over the library that records its calls (tests/test_engine_tensor_contract.py).

The placed run has ten parameters (the gain run's nine and the span table), the statistics run seven."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import window_gain_oracle as go
import window_placed_oracle as po
from aad_amd import capi
from aad_amd.engine import run_extent
from test_engine_tensor_contract import CH, FRAMES, W, CpuEngine, FakeLib, _header, ragged_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "aad_hip.h")


# ---- the symbols -------------------------------------------------------------------------------------------------------------------
def _prototype(text, name):
    m = re.search(r"AADApiResult\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m is not None, name
    return m.group(1)


def test_symbols_are_declared():
    text = open(HEADER).read()
    flowed = re.sub(r"\s*\n \*\s*", " ", text)
    scope = flowed[flowed.index("Out of scope, deliberately"):]
    for phrase in ("int16 rows", "both rows and statistics", "more than one span per row", "loops a short stream"):
        assert phrase in scope[:600], phrase  # the header states what is out of scope
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    placed = _prototype(text, "AADHip_WindowDecodePlanRunPlaced")
    assert len(placed.split(",")) == 10
    assert "const struct AADHipWindowSpan *device_spans" in placed and placed.split(",")[-1].split()[-2:] == ["int32_t", "mode"]
    assert placed.index("device_windows") < placed.index("device_spans") < placed.index("frames_per_window")
    stats = _prototype(text, "AADHip_WindowDecodePlanRunPlacedStats")
    assert len(stats.split(",")) == 7
    assert "const struct AADHipWindowSpan *device_spans" in stats and "struct AADHipRowStats *device_stats" in stats
    assert "sample_type" not in stats and "device_out" not in stats
    s = re.search(r"struct\s+AADHipWindowSpan\s*\{([^}]*)\}", text)
    assert re.findall(r"uint64_t\s+(\w+)\s*;", s.group(1)) == ["num_frames", "out_frame"]
    assert {"AADHip_WindowDecodePlanRunPlaced", "AADHip_WindowDecodePlanRunPlacedStats"} <= set(capi.HIP_SYMBOLS)
    assert C.sizeof(capi.AADHipWindowSpan) == 16
    assert [f[0] for f in capi.AADHipWindowSpan._fields_] == ["num_frames", "out_frame"]


def test_prototypes_are_declared_on_the_library():
    lib = capi.load_library()
    fn = lib.AADHip_WindowDecodePlanRunPlaced
    assert len(fn.argtypes) == 10 and fn.argtypes[-1] is C.c_int32 and fn.argtypes[5] is C.c_uint32 and fn.restype is C.c_int
    fn = lib.AADHip_WindowDecodePlanRunPlacedStats
    assert len(fn.argtypes) == 7 and fn.argtypes[5] is C.c_uint32 and fn.restype is C.c_int


# ---- the oracle, by hand -----------------------------------------------------------------------------------------------------------
def _rows(values):
    return (np.array(values, dtype=np.float32) / np.float32(32768.0)).reshape(1, 1, -1)


def test_span_frames_by_hand():
    assert po.span_frames(5, 0, 8) == 5 and po.span_frames(8, 0, 8) == 8 and po.span_frames(9, 0, 8) == 8
    assert po.span_frames(5, 6, 8) == 2 and po.span_frames(5, 7, 8) == 1 and po.span_frames(5, 8, 8) == 0
    assert po.span_frames(0, 3, 8) == 0 and po.span_frames(2 ** 64 - 1, 1, 8) == 7 and po.span_frames(3, 2 ** 63, 8) == 0
    assert po.span_frames(-1, 1, 8) == 7 and po.span_frames(3, -1, 8) == 0  # int64 values wrap
    assert po.span_frames(2 ** 64 - 1, 2 ** 64 - 1, 8) == 0


def test_oracle_on_hand_computed_cases():
    samples = [16384, -16384, 0, 8192, 1, 2, 3, 4]  # 0.5, -0.5, 0, 0.25, ...
    one, minus = np.ones(1, dtype=np.float32), -np.ones(1, dtype=np.float32)
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    # STORE: the first three frames at element 2 of a row of 8; +0 everywhere else, also under a negative gain
    got = po.placed_expected(_rows(samples), [(3, 2)], minus, "float32")
    assert got.tolist() == [[[0, 0, f32(-0.5), f32(0.5), 0x80000000, 0, 0, 0]]]  # -1 * +0 = -0 INSIDE the span, +0 outside
    got = po.placed_expected(_rows(samples), [(3, 2)], minus, "float16")
    assert got.tolist() == [[[0, 0, 0xB800, 0x3800, 0x8000, 0, 0, 0]]]
    # ADD: -0 and a signalling NaN outside the span survive, inside -0 + +0 = +0
    snan, nzero = 0x7F800001, 0x80000000
    old = np.array([[[nzero, snan, nzero, f32(1.0), f32(0.25), nzero, snan, 7]]], dtype=np.uint32)
    got = po.placed_expected(_rows(samples), [(3, 2)], one, "float32", old)
    assert got.tolist() == [[[nzero, snan, f32(0.5), f32(0.5), f32(0.25), nzero, snan, 7]]]
    assert old[0, 0, 2] == nzero  # the caller's array is not written
    old16 = np.array([[[0x8000, 0x7C01, 0x8000, 0x3C00, 0x3400, 0x8000, 0x7C01, 7]]], dtype=np.uint16)
    got = po.placed_expected(_rows(samples), [(3, 2)], one, "float16", old16)
    assert got.tolist() == [[[0x8000, 0x7C01, 0x3800, 0x3800, 0x3400, 0x8000, 0x7C01, 7]]]
    # clipping: o = 6 leaves two frames; o >= T and L = 0 leave nothing
    got = po.placed_expected(_rows(samples), [(5, 6)], 2 * one, "float32")
    assert got.tolist() == [[[0, 0, 0, 0, 0, 0, f32(1.0), f32(-1.0)]]]
    for span in ((5, 8), (0, 3), (3, 2 ** 63), (3, -1)):
        assert not po.placed_expected(_rows(samples), [span], minus, "bfloat16").any()
        assert np.array_equal(po.placed_expected(_rows(samples), [span], minus, "float32", old), old)
    # no table and (T, 0): the gain run
    for spans in (None, [(8, 0)], [(2 ** 64 - 1, 0)]):
        assert np.array_equal(po.placed_expected(_rows(samples), spans, 3 * one, "bfloat16"), go.gain_expected(_rows(samples), 3 * one, "bfloat16"))


def test_stats_oracle_on_hand_computed_cases():
    rows = np.array([[[3, -4, 5, -32768, 1, 0, 0, 0]]], dtype=np.int16)
    windows = [(0, 10)]
    st = lambda spans, lengths=(15,): po.placed_stats_expected(rows, list(lengths), windows, spans)[0, 0].tolist()
    assert st(None) == [9 + 16 + 25 + 2 ** 30 + 1, 3 + 4 + 5 + 32768 + 1, 32768, 5]
    assert st([(8, 0)]) == st(None)
    assert st([(3, 0)]) == [50, 12, 5, 3] and st([(3, 4)]) == [50, 12, 5, 3]  # the place does not matter to the levels
    assert st([(7, 6)]) == [25, 7, 4, 2]  # clipped to two frames
    assert st([(0, 0)]) == [0, 0, 0, 0] and st([(3, 8)]) == [0, 0, 0, 0]
    assert st([(8, 0)], lengths=(12,))[3] == 2 and st([(1, 0)], lengths=(12,))[3] == 1 and st([(4, 0)], lengths=(10,))[3] == 0
    assert rows[0, 0, 3] == -32768  # the caller's array is not written


# ---- aad_window_span.h against brute force ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("window_span") / "window_span_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "window_span_driver.cpp")], check=True)
    return str(exe)


def test_span_arithmetic_against_brute_force(driver):
    cases = []
    for frames in (1, 2, 15, 16, 17, 33):
        values = sorted({0, 1, 15, 16, 17, frames - 1, frames, frames + 1, 2 ** 63, 2 ** 64 - 1})
        for spb in (4, 5, 20):
            for spb_min in (m for m in (4, 5, 20) if m <= spb):
                for phase in range(spb):
                    for length in values:
                        for o in values:
                            cases.append((frames, spb, spb_min, phase, length, o))
    assert len(cases) > 20000
    out = subprocess.run([driver], input="".join("%d %d %d %d %d %d\n" % c for c in cases), check=True, capture_output=True,
                         text=True).stdout.splitlines()
    assert len(out) == len(cases)
    seen_fill_only = seen_two_pieces = 0
    for case, line in zip(cases, out):
        frames, spb, spb_min, phase, length, o = case
        le, k, bad, max_tile, crop_elements, fill_elements = (int(v) for v in line.split())
        assert le == po.span_frames(length, o, frames), case
        assert k == (0 if frames == 0 else (frames - 1 + spb_min - 1) // spb_min + 1), case
        assert bad == 0, (case, line)  # every element of [0, T) owned exactly once, crops inside the span, fills outside it
        assert max_tile <= spb, (case, line)
        assert crop_elements == le and fill_elements == frames - le, (case, line)
        seen_fill_only += le == 0 and frames > spb
        seen_two_pieces += 0 < le < frames and o > 0 and o + le < frames
    assert seen_fill_only and seen_two_pieces


# ---- the engine's refusals and routing ---------------------------------------------------------------------------------------------
@pytest.fixture
def engine():
    e = CpuEngine.__new__(CpuEngine)
    e.torch, e.lib, e.device, e._ctx = torch, FakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def _plan(e):
    d = ragged_table()
    plan = e.window_decode_plan(_header(), d)
    good = dict(data=torch.zeros(run_extent("images", d), dtype=torch.uint8), windows=torch.zeros((W, 2), dtype=torch.int64))
    return plan, good


def test_without_spans_the_calls_are_those_of_today(engine):
    plan, good = _plan(engine)
    run = lambda **kw: plan.run(good["data"], good["windows"], FRAMES, **kw)
    run()
    run(spans=None)
    run(dtype=torch.int16, spans=None)
    run(stats=True, spans=None)
    run(stats=True, rows=False, spans=None)
    run(gain=torch.ones(W), spans=None)
    run(out=torch.zeros((W, CH, FRAMES)), accumulate=True, spans=None)
    assert [c[0] for c in engine.lib.runs()] == ["AADHip_WindowDecodePlanRun"] * 3 + ["AADHip_WindowDecodePlanRunStats"] * 2 + \
        ["AADHip_WindowDecodePlanRunGain"] * 2
    assert len(engine.lib.last("AADHip_WindowDecodePlanRun")) == 7
    assert len(engine.lib.last("AADHip_WindowDecodePlanRunStats")) == 8
    assert len(engine.lib.last("AADHip_WindowDecodePlanRunGain")) == 9


def test_span_runs_hand_over_the_table(engine):
    plan, good = _plan(engine)
    spans = torch.tensor([[FRAMES, 0], [3, 2], [0, 0], [-1, 1]], dtype=torch.int64)
    gain = torch.ones(W)
    out = plan.run(good["data"], good["windows"], FRAMES, torch.bfloat16, spans=spans)
    assert out.dtype == torch.bfloat16 and out.shape == (W, CH, FRAMES)
    args = engine.lib.last("AADHip_WindowDecodePlanRunPlaced")
    assert args[1:] == (good["data"].data_ptr(), W, good["windows"].data_ptr(), spans.data_ptr(), FRAMES, capi.SAMPLE_BFLOAT16,
                        out.data_ptr(), None, 0)
    assert plan.run(good["data"], good["windows"], FRAMES, torch.bfloat16, out=out, gain=gain, accumulate=True, spans=spans) is out
    assert engine.lib.last("AADHip_WindowDecodePlanRunPlaced")[-3:] == (out.data_ptr(), gain.data_ptr(), 1)
    stats = plan.run(good["data"], good["windows"], FRAMES, stats=True, rows=False, spans=spans)
    assert stats.dtype == torch.int64 and stats.shape == (W, CH, 4)
    args = engine.lib.last("AADHip_WindowDecodePlanRunPlacedStats")
    assert args[1:] == (good["data"].data_ptr(), W, good["windows"].data_ptr(), spans.data_ptr(), FRAMES, stats.data_ptr())
    # a non-contiguous table is copied under ordered=True, as the window table is
    wide = torch.zeros((W, 4), dtype=torch.int64)
    plan.run(good["data"], good["windows"], FRAMES, spans=wide[:, ::2])
    assert engine.lib.last("AADHip_WindowDecodePlanRunPlaced")[4] not in (wide.data_ptr(), None)
    assert [c[0] for c in engine.lib.runs()] == ["AADHip_WindowDecodePlanRunPlaced"] * 2 + ["AADHip_WindowDecodePlanRunPlacedStats"] + \
        ["AADHip_WindowDecodePlanRunPlaced"]


def test_refusals_reach_no_run(engine):
    plan, good = _plan(engine)
    run = lambda **kw: plan.run(good["data"], good["windows"], FRAMES, **kw)
    spans = torch.zeros((W, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match="int16"):
        run(dtype=torch.int16, spans=spans)
    with pytest.raises(ValueError, match="int16"):
        run(dtype=torch.int16, out=torch.zeros((W, CH, FRAMES), dtype=torch.int16), spans=spans)
    with pytest.raises(ValueError, match="both rows and statistics"):
        run(stats=True, spans=spans)
    with pytest.raises(ValueError, match="both rows and statistics"):
        run(stats=torch.zeros((W, CH, 4), dtype=torch.int64), out=torch.zeros((W, CH, FRAMES)), spans=spans)
    with pytest.raises(ValueError, match="statistics-only run"):
        run(stats=True, rows=False, gain=torch.ones(W), spans=spans)  # the gain run's own refusal stays
    with pytest.raises(ValueError, match="spans: shape"):
        run(spans=torch.zeros((W + 1, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="spans: shape"):
        run(spans=torch.zeros((W, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match="spans: shape"):
        run(spans=torch.zeros((2 * W,), dtype=torch.int64))
    with pytest.raises(ValueError, match="spans: dtype torch.int64"):
        run(spans=spans.to(torch.int32))
    with pytest.raises(ValueError, match="spans: dtype torch.int64"):
        run(stats=True, rows=False, spans=spans.to(torch.float32))
    with pytest.raises(ValueError, match="spans: a tensor on the engine's device"):
        run(spans=torch.empty((W, 2), dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError, match="spans: a torch tensor"):
        run(spans=[[FRAMES, 0]] * W)
    with pytest.raises(ValueError, match="spans: a contiguous tensor"):
        plan.run(good["data"], good["windows"], FRAMES, spans=torch.zeros((W, 4), dtype=torch.int64)[:, ::2], ordered=False)
    assert engine.lib.runs() == []
