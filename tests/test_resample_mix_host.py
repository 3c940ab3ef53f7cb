"""Resampled rows with a gain, spans and level statistics (AADHip_ResamplerRunGain, AADHip_ResamplerRunStats; include/aad_hip.h),
what can be checked without a device:
  * the two symbols: prototypes in include/aad_hip.h, HIP_SYMBOLS, argtypes, the refusal of a null handle;
  * aad_amd/csrc/aad_resample.h - resample_output_count and the span clip - built with g++ into tests/resample_mix_driver.cpp and
    held against a brute force over n;
  * tests/resample_mix_oracle.py pinned on hand-computed cases: rails, clamps, the signed zeros of a row without a bank;
  * the engine's routing and refusals over the library that records its calls (tests/test_resample_host.py's ResampleFakeLib)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resample_mix_oracle as mo
import resample_oracle as ro
from aad_amd import capi
from test_engine_tensor_contract import CH, FRAMES, W, CpuEngine, header_bytes
from test_resample_host import RATIOS, T_SRC, ResampleFakeLib, _setup

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "aad_hip.h")
ARGUMENTS = {"AADHip_ResamplerRunGain": 12, "AADHip_ResamplerRunStats": 12}
PLAIN = ["AADHip_ResamplerSourceFrames", "AADHip_ResamplerResolve", "AADHip_WindowDecodePlanRun", "AADHip_ResamplerRun"]


# ---- the symbols -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, count in ARGUMENTS.items():
        m = re.search(r"AADApiResult\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m is not None, name
        assert len(m.group(1).split(",")) == count, name
        assert name in capi.HIP_SYMBOLS
    gain = re.search(r"AADHip_ResamplerRunGain\s*\(([^;]*)\)\s*;", text).group(1)
    assert gain.index("device_lanes") < gain.index("device_spans") < gain.index("sample_type") < gain.index("device_gain") < gain.index("mode")
    stats = re.search(r"AADHip_ResamplerRunStats\s*\(([^;]*)\)\s*;", text).group(1)
    assert stats.index("device_lanes") < stats.index("device_source_stats") < stats.index("device_spans") < stats.index("sample_type") \
        < stats.index("device_out") < stats.index("device_stats")


def test_prototypes_are_declared_on_the_library():
    lib = capi.load_library()
    for name, count in ARGUMENTS.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == count and fn.restype is C.c_int, name
    assert lib.AADHip_ResamplerRunGain.argtypes[1] is C.c_uint64 and lib.AADHip_ResamplerRunGain.argtypes[11] is C.c_int32
    assert lib.AADHip_ResamplerRunStats.argtypes[9] is C.c_int32
    # no device is needed to be refused for a missing handle
    bad = capi.AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_ResamplerRunGain(None, 1, 1, None, 1, None, None, 1, capi.SAMPLE_FLOAT32, None, None, 0) == bad
    assert lib.AADHip_ResamplerRunStats(None, 1, 1, None, 1, None, None, None, 1, capi.SAMPLE_INT16, None, None) == bad


# ---- aad_resample.h against brute force ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("resample_mix") / "resample_mix_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "resample_mix_driver.cpp")], check=True)
    return str(exe)


def _ask(driver, lines):
    out = subprocess.run([driver], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines)
    return out


def test_output_count_against_brute_force(driver):
    shapes = [ro.reduce_ratio(*r) for r in RATIOS]
    shapes = [(L, M, ro.taps(L, M)) for L, M in shapes]
    out = _ask(driver, ["sweep %d %d %d %d" % (L, M, K, K + 20) for L, M, K in shapes])
    checked = 0
    for (L, M, K), line in zip(shapes, out):
        got = iter(int(v) for v in line.split())
        n = np.arange(300)
        centre = n * M // L
        for c_src in range(K + 41):
            c = min(c_src, K + 20)  # never more than the source row's length
            for shift in range(K // 2):
                had = shift + centre < c
                for le in (0, 1, 7, 300):
                    want = int(had[:le].sum())
                    assert next(got) == want == mo.output_count(c_src, K + 20, shift, L, M, le), (L, M, c_src, shift, le)
                    checked += 1
        assert next(got, None) is None
    assert checked > 40000


def test_span_clip_and_large_counts(driver):
    asks = [("span 257 0 257", 257), ("span 0 0 257", 0), ("span 5 0 257", 5), ("span 257 1 257", 256), ("span 10 256 257", 1),
            ("span 10 257 257", 0), ("span 10 %d 257" % (1 << 40), 0), ("span %d 3 257" % (2 ** 64 - 1), 254),
            ("span %d %d 257" % (2 ** 64 - 1, 2 ** 64 - 1), 0),
            # 64-bit arithmetic: c - shift < 2^32 and L <= 1024; M up to 2^31
            ("count 4294967295 4294967295 0 1024 1 4294967295", 4294967295), ("count 4294967295 4294967295 0 1024 1023 1000", 1000),
            ("count 4294967295 4294967295 255 1 2147483647 4294967295", 2), ("count %d 100 7 3 1 4294967295" % (2 ** 64 - 1), 279),
            ("count 7 100 7 3 1 50", 0), ("count 8 100 7 3 1 50", 3)]
    out = _ask(driver, [a for a, _ in asks])
    assert [int(v) for v in out] == [w for _, w in asks]
    for (ask, want) in asks:
        v = [int(t) for t in ask.split()[1:]]
        if ask.startswith("count"):
            assert mo.output_count(*v) == want
            if v[5] <= 1000:
                assert mo.output_count_brute(*v) == want


# ---- the oracle, by hand -----------------------------------------------------------------------------------------------------------
def test_oracle_rail_through_3_1_and_1_3():
    x = np.full(2000, -32768, dtype=np.int16)
    for L, M in ((3, 1), (1, 3)):
        h = ro.bank(L, M)
        for le in (257, 40):
            acc = ro.fir(x, 100, 257, L, M, h)[None, None, :]  # every tap inside the stream
            assert (acc == -(1 << 29)).all()
            spans = None if le == 257 else np.array([[le, 9]], dtype=np.int64)
            rec = mo.expected_stats(acc, spans, np.array([le]))
            assert rec.tolist() == [[[le << 30, le * 32768, 32768, le]]]
            bits = mo.expected_rows(acc, spans, None, "float32")
            assert (bits[0, 0, (0 if spans is None else 9):][:le] == np.float32(-1.0).view(np.uint32)).all()


def test_oracle_square_wave_clamps_in_int16_and_passes_one_in_float():
    x = np.tile(np.repeat(np.array([32767, -32767], dtype=np.int16), 6), 60)
    h = ro.bank(3, 1)
    acc = ro.fir(x, 48, 257, 3, 1, h)
    assert acc.max() > 32767 * 16384 + 8192 and acc.min() < -32768 * 16384 - 8192  # the overshoot of the band limit
    v = ro.convert(acc, "int16")
    assert v.max() == 32767 and v.min() == -32768
    f = mo.float_rows(acc[None, None, :])
    assert f.max() > 1.0 and f.min() < -1.0
    rec = mo.expected_stats(acc[None, None, :], None, np.array([257]))
    assert rec[0, 0, 2] == 32768 and rec[0, 0, 0] == int((v.astype(np.int64) ** 2).sum())


def test_oracle_signed_zeros_of_a_row_without_a_bank():
    acc = np.zeros((1, 2, 10), dtype=np.int64)
    spans = np.array([[5, 3]], dtype=np.int64)
    for name, minus in (("float32", 0x80000000), ("float16", 0x8000), ("bfloat16", 0x8000)):
        bits = mo.expected_rows(acc, spans, np.array([-1.0], dtype=np.float32), name)
        assert (bits[0, :, 3:8] == minus).all() and (bits[0, :, :3] == 0).all() and (bits[0, :, 8:] == 0).all()
        old = np.full(bits.shape, minus, dtype=bits.dtype)  # ADD: old -0 plus -0 stays -0 inside, and is not touched outside
        assert (mo.expected_rows(acc, spans, np.array([-1.0], dtype=np.float32), name, old) == minus).all()
        plus = mo.expected_rows(acc, spans, np.array([1.0], dtype=np.float32), name, old)
        assert (plus[0, :, 3:8] == 0).all() and (plus[0, :, :3] == minus).all()


def test_oracle_counts_by_hand():
    banks = [(3, 1, ro.bank(3, 1)), (1, 3, ro.bank(1, 3))]
    select = [[0, 1]]
    lengths = [100]
    windows = np.array([(0, 0), (0, 90), (0, 99), (0, 100), (0, 90), (1, 0), (0, 90)], dtype=np.int64)
    variant = np.array([0, 0, 0, 0, 1, 0, 2], dtype=np.int64)
    counts = mo.expected_counts(lengths, windows, variant, select, banks, 40, None)
    # 3/1: frame 90 + n div 3 < 100 for n < 30; 1/3: 90 + 3 n < 100 for n < 4
    assert counts.tolist() == [40, 30, 3, 0, 4, 0, 0]
    spans = np.array([(10, 0), (40, 20), (2, 39), (5, 0), (3, 0), (5, 0), (5, 0)], dtype=np.int64)
    assert mo.expected_counts(lengths, windows, variant, select, banks, 40, spans).tolist() == [10, 20, 1, 0, 3, 0, 0]


def test_witness_search_finds_each_kind():
    rng = np.random.default_rng(5)
    accs = rng.integers(-(1 << 28), 1 << 28, size=64)
    for name in ("float32", "float16", "bfloat16"):
        for kind in mo.KINDS:
            if (name, kind) == ("float32", "double"):
                continue
            i, g, old = mo.craft(kind, name, accs)
            assert mo.differs(kind, name, accs[i], g, old)
    # a power of two as the gain is exact all the way: no kind reports it
    assert not mo.differs("double", "float16", accs, np.float32(0.5)).any()
    assert not mo.differs("exact", "float32", accs[np.abs(accs) < 1 << 24], np.float32(1.2345)).any()


# ---- the engine, over the library that records its calls ------------------------------------------------------------------------------
@pytest.fixture
def engine():
    e = CpuEngine.__new__(CpuEngine)
    e.torch, e.lib, e.device, e._ctx = torch, ResampleFakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def _names(e, before):
    return [c[0] for c in e.lib.calls[before:]]


def test_the_plain_call_is_unchanged(engine):
    plan, res, good = _setup(engine)
    before = len(engine.lib.calls)
    out = res.run(plan, good["data"], good["windows"], FRAMES, variant=good["variant"], dtype=torch.float16, out=good["out"])
    assert out is good["out"] and _names(engine, before) == PLAIN
    run = engine.lib.last("AADHip_ResamplerRun")
    assert run[4] == T_SRC and run[6:] == (FRAMES, capi.SAMPLE_FLOAT16, good["out"].data_ptr())


def test_call_order_for_each_argument_combination(engine):
    plan, res, good = _setup(engine)
    gain = torch.ones(W, dtype=torch.float32)
    spans = torch.zeros((W, 2), dtype=torch.int64)
    rows32 = torch.zeros((W, CH, FRAMES), dtype=torch.float32)
    with_gain = PLAIN[:3] + ["AADHip_ResamplerRunGain"]
    with_stats = PLAIN[:2] + ["AADHip_WindowDecodePlanRunStats", "AADHip_ResamplerRunStats"]
    for kwargs, names in ((dict(gain=gain), with_gain), (dict(accumulate=True, out=rows32), with_gain), (dict(spans=spans), with_gain),
                          (dict(gain=gain, accumulate=True, spans=spans, out=rows32), with_gain),
                          (dict(stats=True), with_stats), (dict(stats=True, rows=False), with_stats),
                          (dict(stats=True, rows=False, spans=spans), with_stats)):
        before = len(engine.lib.calls)
        got = res.run(plan, good["data"], good["windows"], FRAMES, **kwargs)
        assert _names(engine, before) == names, kwargs
        resolve = engine.lib.last("AADHip_ResamplerResolve")
        if names is with_gain:
            decode = engine.lib.last("AADHip_WindowDecodePlanRun")
            call = engine.lib.last("AADHip_ResamplerRunGain")
            assert list(call[:6]) == [res.handle, W, CH, decode[6], T_SRC, resolve[6]]
            assert call[6] == (spans.data_ptr() if "spans" in kwargs else None)
            assert call[7:10] == (FRAMES, capi.SAMPLE_FLOAT32, got.data_ptr())
            assert call[10] == (gain.data_ptr() if "gain" in kwargs else None)
            assert call[11] == (capi.WINDOW_GAIN_ADD if kwargs.get("accumulate") else capi.WINDOW_GAIN_STORE)
            if "out" in kwargs:
                assert got is rows32
        else:
            decode = engine.lib.last("AADHip_WindowDecodePlanRunStats")
            assert list(decode[:6]) == [plan.handle, good["data"].data_ptr(), W, resolve[5], T_SRC, capi.SAMPLE_INT16]
            call = engine.lib.last("AADHip_ResamplerRunStats")
            # the source batch's own table is handed on
            assert list(call[:7]) == [res.handle, W, CH, decode[6], T_SRC, resolve[6], decode[7]]
            assert call[7] == (spans.data_ptr() if "spans" in kwargs else None) and call[8:10] == (FRAMES, capi.SAMPLE_FLOAT32)
            if kwargs.get("rows", True):
                rows, table = got
                assert call[10] == rows.data_ptr() and rows.shape == (W, CH, FRAMES)
            else:
                table = got
                assert call[10] is None
            assert call[11] == table.data_ptr() and table.dtype == torch.int64 and table.shape == (W, CH, 4)
    # a table of the caller's
    table = torch.zeros((W, CH, 4), dtype=torch.int64)
    assert res.run(plan, good["data"], good["windows"], FRAMES, stats=table, rows=False) is table


def test_decode_source_once_then_several_fir_runs(engine):
    plan, res, good = _setup(engine)
    before = len(engine.lib.calls)
    source = res.decode_source(plan, good["data"], good["windows"], FRAMES, variant=good["variant"], stats=True)
    assert _names(engine, before) == PLAIN[:2] + ["AADHip_WindowDecodePlanRunStats"]
    assert source.source_frames == T_SRC and source.rows.shape == (W, CH, T_SRC) and source.rows.dtype == torch.int16
    assert source.lanes.shape == (W, 2) and source.lanes.dtype == torch.int32 and source.stats.shape == (W, CH, 4)
    before = len(engine.lib.calls)
    table = res.run_source(source, FRAMES, CH, stats=True, rows=False)
    rows = res.run_source(source, FRAMES, CH, torch.bfloat16)
    res.run_source(source, FRAMES, CH, torch.bfloat16, out=rows, gain=torch.ones(W), accumulate=True)
    assert _names(engine, before) == ["AADHip_ResamplerRunStats", "AADHip_ResamplerRun", "AADHip_ResamplerRunGain"]
    assert table.shape == (W, CH, 4) and rows.dtype == torch.bfloat16
    # a source without statistics cannot feed a statistics run
    plain = res.decode_source(plan, good["data"], good["windows"], FRAMES)
    assert plain.stats is None and engine.lib.calls[-1][0] == "AADHip_WindowDecodePlanRun"
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match="carries no statistics"):
        res.run_source(plain, FRAMES, CH, stats=True, rows=False)
    assert engine.lib.calls[before:] == []


def _corpus(rates):
    data = torch.zeros((len(rates), 64), dtype=torch.uint8)
    for row, rate in enumerate(rates):
        head = bytearray(header_bytes(CH, 100))
        head[18:22] = int(rate).to_bytes(4, "big")
        data[row, :31] = torch.frombuffer(head, dtype=torch.uint8)
    return data


def test_mix_windows_resampled_decodes_each_corpus_once(engine):
    signal, noise = _corpus((16000, 48000)), _corpus((48000, 44100, 16000))
    windows = torch.zeros((W, 2), dtype=torch.int64)
    spans = torch.zeros((W, 2), dtype=torch.int64)
    for noise_spans in (None, spans):
        before = len(engine.lib.calls)
        rows, gains = engine.mix_windows_resampled((signal, 64, windows), (noise, 64, windows), FRAMES, 6.0, 16000,
                                                   dtype=torch.bfloat16, noise_spans=noise_spans)
        calls = engine.lib.calls[before:]
        names = [c[0] for c in calls]
        for name in ("AADHip_ResamplerResolve", "AADHip_WindowDecodePlanRunStats", "AADHip_ResamplerRunStats", "AADHip_ResamplerRunGain"):
            assert names.count(name) == 2, name
        assert "AADHip_WindowDecodePlanRun" not in names and "AADHip_ResamplerRun" not in names
        assert max(names.index("AADHip_WindowDecodePlanRunStats"), names.index("AADHip_ResamplerResolve")) \
            < names.index("AADHip_ResamplerRunStats") < names.index("AADHip_ResamplerRunGain")
        decodes = [c[1] for c in calls if c[0] == "AADHip_WindowDecodePlanRunStats"]
        levels = [c[1] for c in calls if c[0] == "AADHip_ResamplerRunStats"]
        store, add = [c[1] for c in calls if c[0] == "AADHip_ResamplerRunGain"]
        # each FIR run reads its side's one source batch and that batch's own statistics
        for side, (decode, level, run) in enumerate(zip(decodes, levels, (store, add))):
            assert level[3] == run[3] == decode[6] and level[6] == decode[7] and level[10] is None
        assert decodes[0][6] != decodes[1][6]
        assert levels[0][7] is None and levels[1][7] == (None if noise_spans is None else spans.data_ptr())
        assert store[11] == capi.WINDOW_GAIN_STORE and add[11] == capi.WINDOW_GAIN_ADD
        assert store[9] == add[9] == rows.data_ptr() and store[8] == add[8] == capi.SAMPLE_BFLOAT16
        assert store[6] is None and add[6] == (None if noise_spans is None else spans.data_ptr())
        assert add[10] == gains.data_ptr() and store[10] is not None
        assert rows.shape == (W, CH, FRAMES) and rows.dtype == torch.bfloat16 and gains.shape == (W,) and gains.dtype == torch.float32
        assert names[-4:] == ["AADHip_ResamplerDestroy", "AADHip_ResamplerDestroy", "AADHip_WindowDecodePlanDestroy",
                              "AADHip_WindowDecodePlanDestroy"]
    # the two resamplers hold their own corpus's ratios
    creates = [c[1] for c in engine.lib.calls if c[0] == "AADHip_ResamplerCreate"][-2:]
    assert [[(r.up, r.down) for r in c[2]][:c[1]] for c in creates] == [[(1, 1), (1, 3)], [(1, 3), (160, 441), (1, 1)]]


def test_levels_and_rows_of_the_engine_calls(engine):
    data = _corpus((16000, 48000))
    windows = torch.zeros((W, 2), dtype=torch.int64)
    spans = torch.zeros((W, 2), dtype=torch.int64)
    before = len(engine.lib.calls)
    table = engine.window_levels_resampled(data, 64, windows, FRAMES, 16000, spans=spans)
    names = _names(engine, before)
    assert names.count("AADHip_ResamplerRunStats") == 1 and "AADHip_ResamplerRun" not in names and table.shape == (W, CH, 4)
    assert engine.lib.last("AADHip_ResamplerRunStats")[7] == spans.data_ptr() and engine.lib.last("AADHip_ResamplerRunStats")[10] is None
    before = len(engine.lib.calls)
    rows, table = engine.decode_windows_resampled(data, 64, windows, FRAMES, 16000, return_stats=True)
    assert "AADHip_ResamplerRunStats" in _names(engine, before) and rows.shape == (W, CH, FRAMES) and table.shape == (W, CH, 4)
    gain = torch.ones(W, dtype=torch.float32)
    out = torch.zeros((W, CH, FRAMES), dtype=torch.float16)
    before = len(engine.lib.calls)
    got = engine.decode_windows_resampled(data, 64, windows, FRAMES, 16000, dtype=torch.float16, out=out, gain=gain, accumulate=True,
                                          spans=spans)
    call = engine.lib.last("AADHip_ResamplerRunGain")
    assert got is out and call[6] == spans.data_ptr() and call[9:] == (out.data_ptr(), gain.data_ptr(), capi.WINDOW_GAIN_ADD)
    with pytest.raises(ValueError, match="rate and speeds"):
        engine.window_levels_resampled(data, 64, windows, FRAMES, 0)
    with pytest.raises(ValueError, match="rate and speeds"):
        engine.mix_windows_resampled((data, 64, windows), (data, 64, windows), FRAMES, 6.0, 16000, speeds=())


def _good(g):
    return dict(gain=torch.ones(W, dtype=torch.float32), spans=torch.zeros((W, 2), dtype=torch.int64),
                stats=torch.zeros((W, CH, 4), dtype=torch.int64), out=torch.zeros((W, CH, FRAMES), dtype=torch.float32))


RULES = [
    (dict(gain="gain", dtype=torch.int16), "gain / accumulate: float rows only"),
    (dict(accumulate=True, out="out", dtype=torch.int16), "gain / accumulate: float rows only"),
    (dict(spans="spans", dtype=torch.int16), "spans: float rows only"),
    (dict(accumulate=True), "accumulate=True adds into `out`"),
    (dict(gain="gain", stats=True), "gain / accumulate: no statistics variant"),
    (dict(gain="gain", stats=True, rows=False), "gain / accumulate: no statistics variant"),
    (dict(spans="spans", stats=True), "spans: no run with both rows and statistics"),
    (dict(rows=False), "rows=False is a statistics-only run"),
    (dict(rows=False, stats=True, out="out"), "rows=False writes no rows"),
]
TENSORS = [
    ("gain", dict(), lambda t: t.to(torch.float64), "gain: dtype"),
    ("gain", dict(), lambda t: torch.ones(W + 1, dtype=torch.float32), "gain: shape"),
    ("gain", dict(), lambda t: torch.ones(2 * W, dtype=torch.float32)[::2], "gain: a contiguous tensor"),
    ("gain", dict(), lambda t: torch.ones(W, dtype=torch.float32, device="meta"), "gain: a tensor on the engine's device"),
    ("spans", dict(), lambda t: t.to(torch.int32), "spans: dtype"),
    ("spans", dict(), lambda t: torch.zeros((W + 1, 2), dtype=torch.int64), "spans: shape"),
    ("spans", dict(), lambda t: torch.zeros((W, 2), dtype=torch.int64, device="meta"), "spans: a tensor on the engine's device"),
    ("stats", dict(rows=False), lambda t: t.to(torch.int32), "stats: dtype"),
    ("stats", dict(rows=False), lambda t: torch.zeros((W, CH, 3), dtype=torch.int64), "stats: shape"),
    ("stats", dict(rows=False), lambda t: torch.zeros((W, CH, 8), dtype=torch.int64)[..., ::2], "stats: a contiguous tensor"),
    ("stats", dict(rows=False), lambda t: torch.zeros((W, CH, 4), dtype=torch.int64, device="meta"), "stats: a tensor on the engine's device"),
    ("out", dict(gain="gain"), lambda t: t.to(torch.float16), "out: dtype"),
    ("out", dict(gain="gain"), lambda t: torch.zeros((W, CH, FRAMES + 1)), "out: shape"),
    ("out", dict(gain="gain"), lambda t: torch.zeros((W, CH, FRAMES + 3))[..., :FRAMES], "out: a contiguous tensor"),
]


@pytest.mark.parametrize("kwargs,message", RULES, ids=[r[1].split(":")[0].replace(" ", "_") + str(i) for i, r in enumerate(RULES)])
def test_run_refuses_what_window_decode_refuses(engine, kwargs, message):
    plan, res, good = _setup(engine)
    mine = _good(good)
    kwargs = {k: (mine[v] if isinstance(v, str) else v) for k, v in kwargs.items()}
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match=re.escape(message)):
        res.run(plan, good["data"], good["windows"], FRAMES, **kwargs)
    assert engine.lib.calls[before:] == []  # nothing reached the library


@pytest.mark.parametrize("name,extra,spoil,message", TENSORS, ids=[t[3].replace(": ", "-").replace(" ", "_") for t in TENSORS])
def test_run_refuses_a_tensor_off_its_contract(engine, name, extra, spoil, message):
    plan, res, good = _setup(engine)
    mine = _good(good)
    kwargs = {k: (mine[v] if isinstance(v, str) else v) for k, v in extra.items()}
    kwargs[name] = spoil(mine[name])
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match=message):
        res.run(plan, good["data"], good["windows"], FRAMES, **kwargs)
    assert engine.lib.calls[before:] == []
    # the same through the FIR step alone
    source = res.decode_source(plan, good["data"], good["windows"], FRAMES, stats=True)
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match=message):
        res.run_source(source, FRAMES, CH, **kwargs)
    assert engine.lib.calls[before:] == []


def test_run_source_holds_the_record_to_its_channel_count(engine):
    plan, res, good = _setup(engine)
    source = res.decode_source(plan, good["data"], good["windows"], FRAMES, stats=True)
    before = len(engine.lib.calls)
    for kwargs in (dict(), dict(stats=True, rows=False), dict(gain=torch.ones(W, dtype=torch.float32))):
        with pytest.raises(ValueError, match="source.rows: shape"):
            res.run_source(source, FRAMES, CH + 1, **kwargs)
        with pytest.raises(ValueError, match="source.rows: shape"):
            res.run_source(source, FRAMES, 1, **kwargs)
    short = source._replace(stats=source.stats[:, :1].contiguous())
    with pytest.raises(ValueError, match="source.stats: shape"):
        res.run_source(short, FRAMES, CH, stats=True, rows=False)
    with pytest.raises(ValueError, match="source.rows: shape"):
        res.run_source(source._replace(source_frames=T_SRC + 1), FRAMES, CH)
    with pytest.raises(ValueError, match="source.lanes: dtype"):
        res.run_source(source._replace(lanes=source.lanes.to(torch.int64)), FRAMES, CH)
    with pytest.raises(ValueError, match="source.rows: a contiguous tensor"):
        res.run_source(source._replace(rows=torch.zeros((W, CH, T_SRC + 2), dtype=torch.int16)[..., :T_SRC]), FRAMES, CH)
    assert engine.lib.calls[before:] == []  # nothing reached the library


def test_mix_windows_resampled_refuses_corpora_of_different_channel_counts(engine):
    assert CH == 2
    stereo, mono = _corpus((16000, 48000)), _corpus((48000,))
    mono[:, 12:14] = torch.tensor([0, 1], dtype=torch.uint8)  # num_channels = 1 in the header
    from aad_amd.engine import parse_header
    assert parse_header(bytes(mono[0, :31].numpy())).num_channels == 1
    windows = torch.zeros((W, 2), dtype=torch.int64)
    for signal, noise in ((stereo, mono), (mono, stereo)):
        before = len(engine.lib.calls)
        with pytest.raises(ValueError, match="signal and noise: rows of"):
            engine.mix_windows_resampled((signal, 64, windows), (noise, 64, windows), FRAMES, 6.0, 16000)
        names = _names(engine, before)
        assert not [n for n in names if "Run" in n or "Resolve" in n or "Resampler" in n], names  # nothing launched
        assert names[-2:] == ["AADHip_WindowDecodePlanDestroy", "AADHip_WindowDecodePlanDestroy"]
    # one channel count for both: each side's FIR runs take it
    before = len(engine.lib.calls)
    rows, _ = engine.mix_windows_resampled((stereo, 64, windows), (mono, 64, windows), FRAMES, 6.0, 16000, channels=1)
    assert rows.shape == (W, 1, FRAMES)
    runs = [c[1] for c in engine.lib.calls[before:] if c[0] in ("AADHip_ResamplerRunStats", "AADHip_ResamplerRunGain")]
    assert len(runs) == 4 and all(r[2] == 1 for r in runs)


def test_run_checks_in_the_order_it_always_had(engine):
    plan, res, good = _setup(engine)
    before = len(engine.lib.calls)
    bad_windows, bad_variant = good["windows"].to(torch.int32), good["variant"].to(torch.int32)
    bad_out = torch.zeros((W, CH, FRAMES + 1), dtype=torch.float16)
    with pytest.raises(ValueError, match="resample writes"):
        res.run(plan, good["data"], bad_windows, FRAMES, variant=bad_variant, dtype=torch.float64, out=bad_out)
    with pytest.raises(ValueError, match="windows: dtype"):
        res.run(plan, good["data"], bad_windows, FRAMES, variant=bad_variant, dtype=torch.float16, out=bad_out)
    with pytest.raises(ValueError, match="variant: dtype"):
        res.run(plan, good["data"], good["windows"], FRAMES, variant=bad_variant, dtype=torch.float16, out=bad_out)
    with pytest.raises(ValueError, match="out: shape"):
        res.run(plan, good["data"], good["windows"], FRAMES, variant=good["variant"], dtype=torch.float16, out=bad_out)
    assert engine.lib.calls[before:] == []
