"""Level statistics of reverberated rows (AADHip_ConvolverRunStats, include/aad_hip.h "reverberation"), what can be checked without
a device:
  * the symbol: in the header with 12 arguments, in HIP_SYMBOLS, its argtypes, a null handle refused;
  * aad_amd/csrc/aad_convolve.h's convolve_output_count built with g++ into tests/convolve_stats_driver.cpp and held against a
    brute force over n, shifts up to 2^32 - 1 among them;
  * tests/convolve_stats_oracle.py pinned on hand-computed cases: a 4096-frame row at -32768 under the unit response
    (sum_sq = 2^42, which 32 bits do not hold), a response whose sums pass both rails, a window without a response;
  * the mutants: for the inputs of tests/test_gpu_convolve_stats.py (tests/convolve_stats_cases.py) a record taken from the
    unclamped v, a count that ignores the shift, sums over T instead of Le and an idle wave's stale scratch each change a record,
    and the first item's partial sums left in the scratch change the second item's record;
  * the engine's call order and refusals over the library that records its calls (tests/test_convolve_host.py's)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import convolve_oracle as co
import convolve_stats_cases as cases
import convolve_stats_oracle as so
import window_placed_oracle as po
from aad_amd import capi
from aad_amd.engine import ConvolveSource
from test_convolve_host import T_SRC, ConvolveFakeLib, _setup
from test_engine_tensor_contract import CH, FRAMES, W, CpuEngine, header_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "aad_hip.h")
NAME = "AADHip_ConvolverRunStats"
PLAIN = ["AADHip_ConvolverSourceFrames", "AADHip_ConvolverResolve", "AADHip_WindowDecodePlanRun", "AADHip_ConvolverRun"]
WITH_STATS = PLAIN[:2] + ["AADHip_WindowDecodePlanRunStats", NAME]


# ---- the symbol ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"AADApiResult\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m is not None
    args = m.group(1)
    assert len(args.split(",")) == 12 and NAME in capi.HIP_SYMBOLS
    assert "struct AADHipConvolver *" in args and "struct AADHipConvolveLane *" in args and "struct AADHipRowStats *device_stats" in args
    assert args.index("device_lanes") < args.index("device_source_stats") < args.index("device_spans") < args.index("sample_type") \
        < args.index("device_out") < args.index("device_stats")
    # the resampler's twelve, with the convolver's types
    twin = re.search(r"AADApiResult\s+AADHip_ResamplerRunStats\s*\(([^;]*)\)\s*;", text).group(1)
    same = lambda t: re.sub(r"\s+", " ", t.replace("AADHipResampler", "X").replace("AADHipConvolver", "X").replace("resampler", "x")
                            .replace("convolver", "x").replace("AADHipResampleLane", "L").replace("AADHipConvolveLane", "L")).strip()
    assert same(twin) == same(args)
    whole = open(HEADER).read()
    assert "level statistics of reverberated rows" not in whole
    assert "Out of scope, deliberately: a response per channel, responses past 32768 taps." in whole


def test_prototype_is_declared_on_the_library():
    lib = capi.load_library()
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 12 and fn.restype is C.c_int and fn.argtypes == lib.AADHip_ResamplerRunStats.argtypes
    assert lib.AADHip_ConvolverRunStats(None, 1, 1, None, 1, None, None, None, 1, capi.SAMPLE_INT16, None, None) == \
        capi.AADApiResult.INVALID_ARGUMENT


# ---- convolve_output_count through g++ -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("convolve_stats") / "convolve_stats_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "convolve_stats_driver.cpp")], check=True)
    return str(exe)


def _ask(driver, lines):
    out = subprocess.run([driver], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("t_src", [1, 40, 339])
def test_output_count_against_brute_force(driver, t_src):
    shifts = [0, 1, t_src - 1, t_src, 1 << 31, (1 << 32) - 1]
    lengths = [0, 1, 7, 300]
    line = _ask(driver, ["sweep %d %d %d %s %s" % (t_src, len(shifts), len(lengths), " ".join(map(str, shifts)), " ".join(map(str, lengths)))])[0]
    got = iter(int(v) for v in line.split())
    checked = 0
    for c_src in range(t_src + 4):
        for shift in shifts:
            for le in lengths:
                brute = sum(1 for n in range(le) if shift + n < min(c_src, t_src))  # the source elements shift + n the stream had
                assert next(got) == brute == so.output_count(c_src, t_src, shift, le) == so.output_count_brute(c_src, t_src, shift, le), \
                    (c_src, shift, le)
                checked += 1
    assert next(got, None) is None and checked == (t_src + 4) * 24


def test_output_count_in_64_bits(driver):
    top = (1 << 32) - 1
    asks = [("count %d %d %d %d" % (top, top, top - 1, 300), 1), ("count %d %d %d %d" % (top, top, top, 300), 0),
            ("count %d %d 0 %d" % (top, top, top), top), ("count %d %d %d %d" % ((1 << 64) - 1, top, 1 << 31, top), (1 << 31) - 1),
            ("count %d 100 7 %d" % ((1 << 64) - 1, top), 93), ("count 7 100 7 50", 0), ("count 8 100 7 50", 1), ("count 0 100 0 50", 0),
            ("count 99 100 %d 50" % top, 0)]
    assert [int(v) for v in _ask(driver, [a for a, _ in asks])] == [w for _, w in asks]
    for ask, want in asks:
        assert so.output_count(*[int(t) for t in ask.split()[1:]]) == want


# ---- the oracle, by hand -------------------------------------------------------------------------------------------------------------
def test_oracle_rail_under_the_unit_response():
    taps, q, d = co.quantise([1.0])
    x = np.full(4096, -32768, dtype=np.int16)
    acc = co.sums(x, 0, 4096, taps, d)[None, None, :]
    assert (acc == -32768 * 16384).all()
    rec = so.expected_stats(acc, [q], None, [4096])
    assert rec.tolist() == [[[1 << 42, 4096 * 32768, 32768, 4096]]]
    assert (1 << 42) & 0xFFFFFFFF != 1 << 42  # a 32-bit sum_sq would differ
    u = np.abs(co.to_int16(acc[0, 0], q).astype(np.int64)).astype(np.uint32)
    assert int((u * u).sum(dtype=np.uint32)) != rec[0, 0, 0]
    # sixteen outputs of one thread at the rail: 2^34, past 32 bits before the wave meets
    assert so.record([-32768] * 16, 0)[0] == 1 << 34
    # over a span of 1000 frames, and an empty one
    assert so.expected_stats(acc, [q], np.array([[1000, 7]]), [555]).tolist() == [[[1000 << 30, 1000 * 32768, 32768, 555]]]
    assert so.expected_stats(acc, [q], np.array([[1000, 4096]]), [0]).tolist() == [[[0, 0, 0, 0]]]


def test_oracle_sums_past_both_rails_are_clamped_in_the_record():
    taps, q, d = co.quantise([1.0, 1.0, 1.0])  # an energy above one: 3 x full scale
    assert (taps.tolist(), q, d) == ([16384] * 3, 14, 0)
    x = np.array([32767, 32767, 32767, 0, 0, -32768, -32768, -32768, 5], dtype=np.int16)
    acc = co.sums(x, 0, 9, taps, d)
    assert (acc >> 14).tolist() == [32767, 65534, 98301, 65534, 32767, -32768, -65536, -98304, -65531]
    v = so.values(acc, q).tolist()
    assert v == [32767, 32767, 32767, 32767, 32767, -32768, -32768, -32768, -32768]
    assert so.expected_stats(acc[None, None], [q], None, [9]).tolist() == \
        [[[5 * 32767 ** 2 + 4 * 32768 ** 2, 5 * 32767 + 4 * 32768, 32768, 9]]]
    loose = so.expected_stats(acc[None, None], [q], None, [9], clamp=False)
    assert loose[0, 0, 2] == 98304 and loose[0, 0, 0] > 1 << 34
    # the float row is not clamped: the record is the witness
    assert co.to_float32(acc, q)[2] == np.float32(98301 / 32768)


def test_oracle_window_without_a_response():
    acc = np.zeros((2, 2, 5), dtype=np.int64)
    acc[0] = 16384 * 7
    rec = so.expected_stats(acc, [14, 0], None, [5, 3], has_response=[True, False])
    assert rec[0].tolist() == [[5 * 49, 35, 7, 5]] * 2 and not rec[1].any()
    lengths, responses = [100], [co.quantise([0.0, 1.0, 0.5])]
    windows = np.array([(0, 98), (0, 0), (0, 98), (0, 98), (5, 0), (0, 200)], dtype=np.int64)
    index = np.array([0, 0, 1, -1, 0, 0], dtype=np.int64)
    assert so.stream_counts(lengths, windows, index, responses, 10, None).tolist() == [2, 10, 0, 0, 0, 0]
    assert so.stream_counts(lengths, windows, index, responses, 10, np.array([[1, 0]] * 6)).tolist() == [1, 1, 0, 0, 0, 0]


# ---- the mutants over the GPU file's inputs ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile():
    return cases.tile_case()


def test_the_tile_case_is_what_it_says(tile):
    t = tile
    assert t.frames == 4360 and t.rows.shape == (8, 2, 4360 + 4199)
    assert -(-(t.frames - 4096) // 256) == 2  # two blocks in the second tile: waves 2 and 3 idle
    want = so.expected_stats(t.acc, t.qs, None, cases.counts_of(t, None), t.has_response)
    assert want[2].tolist() == [[4360 << 30, 4360 * 32768, 32768, 3000], [4360 << 30, 4360 * 32768, 32768, 4360]]
    assert want[2, 0, 0] > 1 << 32
    assert t.acc[3, :, :4096].any() and not t.acc[3, :, 4096:].any()  # a loud first tile, a silent second
    assert not want[4].any() and not t.has_response[4]
    assert (np.abs(t.acc[0] >> 14) > 40000).any()  # sums past full scale under the 40-tap response
    counts = cases.counts_of(t, None)
    assert (counts == t.frames).any() and (counts == 0).any() and ((counts > 0) & (counts < t.frames)).any()
    for spans in t.span_sets[1:]:
        le = [c[0] for c in po.clipped(spans, 8, t.frames)]
        assert 0 in le and 3000 in le and 4200 in le and any(4096 < v < t.frames for v in le)


def test_each_mistake_changes_a_record_of_the_tile_case(tile):
    t = tile
    for spans in t.span_sets:
        counts = cases.counts_of(t, spans)
        want = so.expected_stats(t.acc, t.qs, spans, counts, t.has_response)
        unclamped = so.expected_stats(t.acc, t.qs, spans, counts, t.has_response, clamp=False)
        assert (unclamped[..., :3] != want[..., :3]).any()
        no_shift = so.expected_stats(t.acc, t.qs, spans, cases.counts_of(t, spans, ignore_shift=True), t.has_response)
        assert (no_shift[..., 3] != want[..., 3]).any()
        if spans is not None:
            over_row = so.expected_stats(t.acc, t.qs, spans, counts, t.has_response, over_row=True)
            assert (over_row[..., :3] != want[..., :3]).any()
        stale = so.stale_scratch_stats(t.acc, t.qs, spans, counts)
        stale[~t.has_response] = 0
        assert (stale[..., :2] != want[..., :2]).any()
    # without spans the stale slots of waves 2 and 3 reach every loud row with a second tile, the row at the rail among them
    stale = so.stale_scratch_stats(t.acc, t.qs, None, cases.counts_of(t, None))
    want = so.expected_stats(t.acc, t.qs, None, cases.counts_of(t, None), t.has_response)
    assert (stale[[0, 1, 2, 3], :, 0] > want[[0, 1, 2, 3], :, 0]).all()


def test_the_first_items_sums_left_in_the_scratch_change_the_second_items_record():
    h, rows, c_src = cases.item_loop_rows()
    want, v = cases.item_loop_expected(h, rows, c_src)
    taps, q, d = co.quantise(h, cases.ITEM_TAPS - 1)
    for w in (0, 1, 76, 100, 1 << 20, (1 << 20) + 9, cases.ITEM_ROWS - 1):  # the vectorised records against the oracle's sums
        acc = co.sums(rows[w, 0], 0, 1, taps, d)
        assert so.expected_stats(acc[None, None], [q], None, [so.output_count(c_src[w], 40, 0, 1)]).tolist() == want[w:w + 1].tolist()
    second = np.arange(1 << 20, cases.ITEM_ROWS)
    first = second - (1 << 20)  # the item the same workgroup ran before
    assert (v[first] != 0).all()  # every first item leaves sums behind ...
    left = want[second].copy()
    left[:, 0, 0] += want[first, 0, 0]
    left[:, 0, 1] += want[first, 0, 1]
    left[:, 0, 2] = np.maximum(left[:, 0, 2], want[first, 0, 2])
    assert (left[:, 0, :2] != want[second][:, 0, :2]).all()  # ... which would change every second item's record
    assert not want[(1 << 20) + 9, 0, :3].any() and not want[100, 0, :3].any() and (np.abs(v) == 32768).any()


def test_each_mistake_changes_a_record_of_the_corpus_cases():
    """the windows of tests/test_gpu_convolve.py over streams of the corpora's lengths: the counts alone need no decode"""
    from test_gpu_convolve import TAPS, _responses, _windows
    from test_gpu_window_resample import LENGTHS
    for rotate in range(4):
        hs, delays = _responses(rotate, False)
        responses = [co.quantise(h, d) for h, d in zip(hs, delays)]
        assert [len(r[0]) for r in responses] == TAPS
        windows, index = _windows(responses)
        for frames in (257, 1025):
            counts = so.stream_counts(LENGTHS, windows, index, responses, frames, None)
            assert (counts == frames).any() and ((counts > 0) & (counts < frames)).any() and (counts == 0).any()
            assert (so.stream_counts(LENGTHS, windows, index, responses, frames, None, ignore_shift=True) != counts).any()


# ---- the engine, over the library that records its calls ---------------------------------------------------------------------------------
@pytest.fixture
def engine():
    e = CpuEngine.__new__(CpuEngine)
    e.torch, e.lib, e.device, e._ctx = torch, ConvolveFakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def _names(e, before):
    return [c[0] for c in e.lib.calls[before:]]


def test_the_plain_run_makes_the_same_four_calls(engine):
    plan, conv, good = _setup(engine)
    before = len(engine.lib.calls)
    out = conv.run(plan, good["data"], good["windows"], FRAMES, response=good["response"], dtype=torch.float16, out=good["out"])
    assert out is good["out"] and _names(engine, before) == PLAIN
    # a record built by hand, without statistics, serves every run that asks for none
    rows, lanes = torch.zeros((W, CH, T_SRC), dtype=torch.int16), torch.zeros((W, 2), dtype=torch.int32)
    before = len(engine.lib.calls)
    conv.run_source(ConvolveSource(rows, lanes, T_SRC), FRAMES, CH)
    conv.run_source(ConvolveSource(rows, lanes, T_SRC), FRAMES, CH, gain=good["gain"])
    assert [n for n in _names(engine, before) if "Run" in n] == ["AADHip_ConvolverRun", "AADHip_ConvolverRunGain"]


def test_call_order_of_the_runs_with_statistics(engine):
    plan, conv, good = _setup(engine)
    spans = good["spans"]
    for kwargs in (dict(stats=True), dict(stats=True, rows=False, spans=spans), dict(stats=True, rows=False),
                   dict(stats=True, dtype=torch.float16, out=good["out"])):
        before = len(engine.lib.calls)
        got = conv.run(plan, good["data"], good["windows"], FRAMES, response=good["response"], **kwargs)
        assert _names(engine, before) == WITH_STATS, kwargs
        resolve = engine.lib.last("AADHip_ConvolverResolve")
        decode = engine.lib.last("AADHip_WindowDecodePlanRunStats")
        assert list(decode[:6]) == [plan.handle, good["data"].data_ptr(), W, resolve[5], T_SRC, capi.SAMPLE_INT16]
        call = engine.lib.last(NAME)
        assert list(call[:7]) == [conv.handle, W, CH, decode[6], T_SRC, resolve[6], decode[7]]  # the source batch's own table
        assert call[7] == (spans.data_ptr() if "spans" in kwargs else None)
        assert call[8:10] == (FRAMES, capi.SAMPLE_FLOAT16 if "dtype" in kwargs else capi.SAMPLE_FLOAT32)
        if kwargs.get("rows", True):
            rows, table = got
            assert call[10] == rows.data_ptr() and rows.shape == (W, CH, FRAMES)
        else:
            table = got
            assert call[10] is None
        assert call[11] == table.data_ptr() and table.dtype == torch.int64 and table.shape == (W, CH, 4)
    table = torch.zeros((W, CH, 4), dtype=torch.int64)
    assert conv.run(plan, good["data"], good["windows"], FRAMES, stats=table, rows=False) is table
    # one decode, several FIR runs
    source = conv.decode_source(plan, good["data"], good["windows"], FRAMES, response=good["response"], stats=True)
    assert source.stats.shape == (W, CH, 4)
    before = len(engine.lib.calls)
    conv.run_source(source, FRAMES, CH, stats=True, rows=False)
    conv.run_source(source, FRAMES, CH, torch.bfloat16, gain=good["gain"])
    assert [n for n in _names(engine, before) if "Run" in n] == [NAME, "AADHip_ConvolverRunGain"]


def test_one_refusal_per_rule(engine):
    plan, conv, good = _setup(engine)
    run = lambda **k: conv.run(plan, good["data"], good["windows"], FRAMES, **k)
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match="spans: no run with both rows and statistics"):
        run(spans=good["spans"], stats=True)
    with pytest.raises(ValueError, match="gain / accumulate: no statistics variant"):
        run(gain=good["gain"], stats=True)
    with pytest.raises(ValueError, match="rows=False is a statistics-only run"):
        run(rows=False)
    with pytest.raises(ValueError, match="rows=False writes no rows"):
        run(rows=False, stats=True, out=torch.zeros((W, CH, FRAMES)))
    with pytest.raises(ValueError, match="stats: shape"):
        run(stats=torch.zeros((W, CH, 3), dtype=torch.int64), rows=False)
    with pytest.raises(TypeError, match="unexpected keyword argument 'variant'"):
        run(variant=good["response"])
    assert engine.lib.calls[before:] == []
    plain = conv.decode_source(plan, good["data"], good["windows"], FRAMES)
    assert plain.stats is None and engine.lib.calls[-1][0] == "AADHip_WindowDecodePlanRun"
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match="carries no statistics"):
        conv.run_source(plain, FRAMES, CH, stats=True, rows=False)
    rows, lanes = torch.zeros((W, CH, T_SRC), dtype=torch.int16), torch.zeros((W, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="source.stats: shape"):
        conv.run_source(ConvolveSource(rows, lanes, T_SRC, torch.zeros((W, 1, 4), dtype=torch.int64)), FRAMES, CH, stats=True, rows=False)
    assert engine.lib.calls[before:] == []


def _corpus(streams, channels=CH):
    data = torch.zeros((streams, 64), dtype=torch.uint8)
    data[:, :31] = torch.frombuffer(bytearray(header_bytes(channels, 100)), dtype=torch.uint8)
    return data


def test_levels_and_rows_of_the_engine_calls(engine):
    data, windows = _corpus(3), torch.zeros((W, 2), dtype=torch.int64)
    spans, index = torch.zeros((W, 2), dtype=torch.int64), torch.zeros(W, dtype=torch.int64)
    before = len(engine.lib.calls)
    table = engine.window_levels_reverberated(data, 64, windows, FRAMES, [[1.0], [0.25, 0.5]], response=index, spans=spans)
    names = _names(engine, before)
    assert [n for n in names if "Run" in n or "Resolve" in n] == ["AADHip_ConvolverResolve", "AADHip_WindowDecodePlanRunStats", NAME]
    assert names[-2:] == ["AADHip_ConvolverDestroy", "AADHip_WindowDecodePlanDestroy"]
    call = engine.lib.last(NAME)
    assert table.shape == (W, CH, 4) and call[7] == spans.data_ptr() and call[10] is None and call[11] == table.data_ptr()
    before = len(engine.lib.calls)
    rows, table = engine.decode_windows_reverberated(data, 64, windows, FRAMES, [[1.0]], dtype=torch.bfloat16, return_stats=True)
    names = _names(engine, before)
    assert [n for n in names if "Run" in n or "Resolve" in n] == ["AADHip_ConvolverResolve", "AADHip_WindowDecodePlanRunStats", NAME]
    call = engine.lib.last(NAME)
    assert rows.dtype == torch.bfloat16 and call[9:] == (capi.SAMPLE_BFLOAT16, rows.data_ptr(), table.data_ptr())
    # without statistics the call is the one it was
    before = len(engine.lib.calls)
    engine.decode_windows_reverberated(data, 64, windows, FRAMES, [[1.0]])
    assert [n for n in _names(engine, before) if "Run" in n or "Resolve" in n] == PLAIN[1:]
    # a refused argument is found before the convolver is built
    before = len(engine.lib.calls)
    for call, bad, message in ((engine.window_levels_reverberated, dict(spans=spans.to(torch.int32)), "spans: dtype"),
                               (engine.window_levels_reverberated, dict(response=torch.zeros(W + 1, dtype=torch.int64)), "response: shape"),
                               (engine.window_levels_reverberated, dict(delays=[3]), "delays"),
                               (engine.decode_windows_reverberated, dict(return_stats=True, spans=spans), "spans: no run with both rows"),
                               (engine.decode_windows_reverberated, dict(return_stats=True, gain=torch.ones(W)), "no statistics variant")):
        with pytest.raises(ValueError, match=message):
            call(data, 64, windows, FRAMES, [[1.0]], **bad)
    assert not any(c[0].startswith("AADHip_Convolver") for c in engine.lib.calls[before:])


def test_mix_windows_reverberated_with_dry_noise(engine):
    signal, noise = _corpus(2), _corpus(3)
    windows, spans = torch.zeros((W, 2), dtype=torch.int64), torch.zeros((W, 2), dtype=torch.int64)
    index = torch.zeros(W, dtype=torch.int64)
    for noise_spans in (None, spans):
        before = len(engine.lib.calls)
        rows, gains = engine.mix_windows_reverberated((signal, 64, windows), (noise, 64, windows), FRAMES, 6.0, [[1.0], [0.5, 0.25]],
                                                      response=index, dtype=torch.bfloat16, noise_spans=noise_spans)
        calls = engine.lib.calls[before:]
        names = [c[0] for c in calls]
        placed = noise_spans is not None
        level, add = ("AADHip_WindowDecodePlanRunPlacedStats", "AADHip_WindowDecodePlanRunPlaced") if placed else \
            ("AADHip_WindowDecodePlanRunStats", "AADHip_WindowDecodePlanRunGain")
        # one resolve, one decode with statistics, the two FIR runs over it, and the noise plan's two runs
        assert [n for n in names if "Run" in n or "Resolve" in n] == \
            ["AADHip_ConvolverResolve", "AADHip_WindowDecodePlanRunStats", NAME] + ([level] if placed else ["AADHip_WindowDecodePlanRunStats"]) \
            + ["AADHip_ConvolverRunGain", add]
        assert names.count("AADHip_ConvolverCreate") == 1 and "AADHip_ConvolverRun" not in names
        decode = [c[1] for c in calls if c[0] == "AADHip_WindowDecodePlanRunStats"][0]
        levels, store = engine.lib.last(NAME), engine.lib.last("AADHip_ConvolverRunGain")
        assert levels[3] == store[3] == decode[6] and levels[6] == decode[7] and levels[10] is None and levels[7] is None
        assert store[6] is None and store[8:10] == (capi.SAMPLE_BFLOAT16, rows.data_ptr()) and store[11] == capi.WINDOW_GAIN_STORE
        assert store[10] is not None and store[10] != gains.data_ptr()
        added = engine.lib.last(add)
        assert rows.data_ptr() in added and gains.data_ptr() in added  # into the signal's rows: one pointer
        if placed:
            assert spans.data_ptr() in added and spans.data_ptr() in engine.lib.last(level)
        assert rows.shape == (W, CH, FRAMES) and rows.dtype == torch.bfloat16 and gains.shape == (W,) and gains.dtype == torch.float32
        assert names[-3:] == ["AADHip_ConvolverDestroy", "AADHip_WindowDecodePlanDestroy", "AADHip_WindowDecodePlanDestroy"]


def test_mix_windows_reverberated_with_reverberant_noise(engine):
    signal, noise = _corpus(2), _corpus(3)
    windows, spans = torch.zeros((W, 2), dtype=torch.int64), torch.zeros((W, 2), dtype=torch.int64)
    n_index = torch.ones(W, dtype=torch.int64)
    for noise_spans in (None, spans):
        before = len(engine.lib.calls)
        rows, gains = engine.mix_windows_reverberated((signal, 64, windows), (noise, 64, windows), FRAMES, 6.0, [[1.0]],
                                                      noise_responses=[[1.0], [0.5, 0.25, 0.1]], noise_response=n_index, noise_delays=[None, 1],
                                                      noise_spans=noise_spans)
        calls = engine.lib.calls[before:]
        names = [c[0] for c in calls]
        # two resolves, two decodes with statistics and four convolver runs
        for name in ("AADHip_ConvolverCreate", "AADHip_ConvolverResolve", "AADHip_WindowDecodePlanRunStats", NAME, "AADHip_ConvolverRunGain"):
            assert names.count(name) == 2, name
        assert "AADHip_WindowDecodePlanRun" not in names and "AADHip_ConvolverRun" not in names
        assert [n for n in names if n.startswith("AADHip_ConvolverRun")] == [NAME, NAME, "AADHip_ConvolverRunGain", "AADHip_ConvolverRunGain"]
        decodes = [c[1] for c in calls if c[0] == "AADHip_WindowDecodePlanRunStats"]
        levels = [c[1] for c in calls if c[0] == NAME]
        store, add = [c[1] for c in calls if c[0] == "AADHip_ConvolverRunGain"]
        for decode, level, run in zip(decodes, levels, (store, add)):
            assert level[3] == run[3] == decode[6] and level[6] == decode[7] and level[10] is None and level[0] == run[0]
        assert decodes[0][6] != decodes[1][6] and store[0] != add[0]
        assert levels[0][7] is None and levels[1][7] == (None if noise_spans is None else spans.data_ptr())
        assert store[11] == capi.WINDOW_GAIN_STORE and add[11] == capi.WINDOW_GAIN_ADD and store[9] == add[9] == rows.data_ptr()
        assert store[6] is None and add[6] == (None if noise_spans is None else spans.data_ptr()) and add[10] == gains.data_ptr()
        resolves = [c[1] for c in calls if c[0] == "AADHip_ConvolverResolve"]
        assert resolves[0][3] is None and resolves[1][3] == n_index.data_ptr()
        assert rows.dtype == torch.float32 and names[-4:] == ["AADHip_ConvolverDestroy", "AADHip_ConvolverDestroy",
                                                               "AADHip_WindowDecodePlanDestroy", "AADHip_WindowDecodePlanDestroy"]
    creates = [c[1] for c in engine.lib.calls if c[0] == "AADHip_ConvolverCreate"][-2:]
    assert [list(c[3])[:c[1]] for c in creates] == [[1], [1, 3]] and list(creates[1][4]) == [-1, 1]


def test_mix_windows_reverberated_checks_before_it_builds(engine):
    assert CH == 2
    stereo, mono = _corpus(2), _corpus(1, channels=1)
    windows = torch.zeros((W, 2), dtype=torch.int64)
    mix = lambda s=stereo, n=stereo, sw=windows, nw=windows, responses=((1.0,),), **k: \
        engine.mix_windows_reverberated((s, 64, sw), (n, 64, nw), FRAMES, 6.0, [list(r) for r in responses], **k)
    before = len(engine.lib.calls)
    for kwargs, message in ((dict(s=stereo, n=mono), "signal and noise: rows of 2 and 1 channels"), (dict(s=mono, n=stereo), "signal and noise: rows of"),
                            (dict(responses=((),)), "responses"), (dict(delays=[5]), "delays"), (dict(noise_responses=[[]]), "responses"),
                            (dict(noise_response=torch.zeros(W, dtype=torch.int64)), "the noise has no responses"),
                            (dict(dtype=torch.int16), "float rows only"), (dict(dtype=torch.float64), "convolve writes"),
                            (dict(sw=windows.to(torch.int32)), "windows: dtype"), (dict(nw=torch.zeros((W + 1, 2), dtype=torch.int64)), "noise windows: shape"),
                            (dict(response=torch.zeros(W + 1, dtype=torch.int64)), "response: shape"),
                            (dict(noise_spans=torch.zeros((W, 3), dtype=torch.int64)), "noise_spans: shape"),
                            (dict(noise_responses=[[1.0]], noise_response=torch.zeros(W, dtype=torch.int32)), "noise_response: dtype")):
        with pytest.raises(ValueError, match=message):
            mix(**kwargs)
    names = _names(engine, before)
    assert not [n for n in names if "Run" in n or "Resolve" in n or "Convolver" in n], names  # nothing built, nothing launched
    rows, _ = mix(s=stereo, n=mono, channels=1)
    assert rows.shape == (W, 1, FRAMES)
