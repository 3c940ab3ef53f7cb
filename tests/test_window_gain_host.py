"""Window decode with a per-window gain (AADHip_WindowDecodePlanRunGain), what can be checked without a device:
  * the symbol: in include/aad_hip.h and in HIP_SYMBOLS, 9 arguments, the enum's values;
  * tests/window_gain_oracle.py pinned on hand-computed cases, and each of its witnesses confirmed with fractions.Fraction;
  * the vector-path witnesses of every case of tests/test_gpu_window_decode_matrix.py: each confirmed with fractions.Fraction, the
    four classes of a chunk covered per stream and kind, each element on the chunk path by the formula and by a restatement of
    the lane's arithmetic;
  * snr_gains against a float64 computation on crafted tables;
  * the engine's refusals, over the library that records its calls (tests/test_engine_tensor_contract.py)."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import window_gain_oracle as go
from aad_amd import capi
from aad_amd.engine import run_extent, snr_gains
from test_engine_tensor_contract import CH, FRAMES, W, CpuEngine, FakeLib, _header, ragged_table
from window_half_oracle import half_bits_expected

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aad_hip.h")


# ---- the symbol --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_with_nine_arguments():
    text = open(HEADER).read()
    assert "AADHip_WindowDecodePlanRunGain" in capi.HIP_SYMBOLS
    assert "no statistics variant" in text  # the header says where the levels come from
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"AADApiResult\s+AADHip_WindowDecodePlanRunGain\s*\(([^;]*)\)\s*;", text)
    assert m is not None
    args = m.group(1).split(",")
    assert len(args) == 9
    assert "const float *device_gain" in m.group(1) and args[-1].split()[-2:] == ["int32_t", "mode"]
    e = re.search(r"enum\s+AADHipWindowGainMode\s*\{([^}]*)\}", text)
    values = dict(re.findall(r"(AAD_HIP_WINDOW_GAIN_\w+)\s*=\s*(\d+)", e.group(1)))
    assert values == {"AAD_HIP_WINDOW_GAIN_STORE": "0", "AAD_HIP_WINDOW_GAIN_ADD": "1"}
    assert (capi.WINDOW_GAIN_STORE, capi.WINDOW_GAIN_ADD) == (0, 1)


def test_prototype_is_declared_on_the_library():
    lib = capi.load_library()
    fn = lib.AADHip_WindowDecodePlanRunGain
    assert len(fn.argtypes) == 9 and fn.argtypes[-1] is C.c_int32 and fn.restype is C.c_int


# ---- the oracle, by hand -----------------------------------------------------------------------------------------------------------
def _rows(values):
    return (np.array(values, dtype=np.float32) / np.float32(32768.0)).reshape(1, 1, -1)


def test_oracle_on_hand_computed_cases():
    samples = np.array([0, 1, -1, 2049, -257, 32767, -32768, 12345], dtype=np.int16)
    one = np.ones(1, dtype=np.float32)
    for name in ("float16", "bfloat16"):  # gain 1 is the plain half row
        assert np.array_equal(go.gain_expected(_rows(samples), one, name), half_bits_expected(samples.reshape(1, 1, -1), name))
        assert np.array_equal(go.gain_expected(_rows(samples), None, name), half_bits_expected(samples.reshape(1, 1, -1), name))
        assert go.gain_expected(_rows([0]), -one, name).item() == 0x8000      # -1 * +0 = -0
        minus_zero = np.array([[[0x8000]]], dtype=np.uint16)
        assert go.gain_expected(_rows([0]), one, name, minus_zero).item() == 0  # -0 + +0 = +0 ...
        assert go.gain_expected(_rows([0]), -one, name, minus_zero).item() == 0x8000  # ... and -0 + -0 stays
    assert go.gain_expected(_rows([0]), -one, "float32").item() == 0x80000000
    assert go.gain_expected(_rows([0]), one, "float32", np.array([[[0x80000000]]], dtype=np.uint32)).item() == 0
    assert go.gain_expected(_rows([16384]), 3 * one, "float32").item() == 0x3FC00000  # 1.5
    assert go.gain_expected(_rows([16384]), 3 * one, "float16").item() == 0x3E00
    assert go.gain_expected(_rows([16384]), 3 * one, "bfloat16", np.array([[[0x3F80]]], dtype=np.uint16)).item() == 0x4020  # 1 + 1.5
    # a subnormal product: 2^-120 * 3 * 2^-15 = 3 * 2^-135 = 3 * 2^14 units of 2^-149; and one that rounds: 12345 * 2^-135 * 2^-..
    tiny = np.array([2.0 ** -120], dtype=np.float32)
    assert go.gain_expected(_rows([3]), tiny, "float32").item() == 3 << 14
    assert go.gain_expected(_rows([-3]), tiny, "float32").item() == 0x80000000 | (3 << 14)
    tinier = np.array([2.0 ** -136], dtype=np.float32)  # 5 * 2^-151 = 1.25 units -> 1; 7 * 2^-151 = 1.75 -> 2; 6 * 2^-151 = 1.5 -> 2
    assert [go.gain_expected(_rows([v]), tinier, "float32").item() for v in (5, 7, 6, 2)] == [1, 2, 2, 0]
    assert go.gain_expected(_rows([3]), tiny, "float16").item() == 0  # far below binary16


def test_rounding_helpers_agree_with_each_other_and_with_numpy():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-3, 3, 200), rng.uniform(-1, 1, 200) * 2.0 ** -130, rng.uniform(-1, 1, 200) * 2.0 ** -16])
    assert np.array_equal(go.round_f64(x, "float32"), x.astype(np.float32).astype(np.float64))
    assert np.array_equal(go.round_f64(x, "float16"), x.astype(np.float16).astype(np.float64))
    for name in go.DTYPES:
        got = go.round_f64(x, name)
        for v, r in zip(x[::7].tolist(), got[::7].tolist()):
            assert go.round_fraction(Fraction(v), name) == Fraction(r), (name, v)
    assert go.round_fraction(Fraction(2049, 32768), "float16") == Fraction(2048, 32768)  # the ties of the half rows
    assert go.round_fraction(Fraction(259, 32768), "bfloat16") == Fraction(260, 32768)


# ---- the witnesses -----------------------------------------------------------------------------------------------------------------
def test_witnesses_are_witnesses():
    w = go.witnesses()
    counts = {k: len(v) for k, v in w.items()}
    assert all(n >= 8 for n in counts.values()), counts
    fr = lambda v: Fraction(float(v))
    f = lambda sample: Fraction(int(sample), 32768)
    for name in ("float16", "bfloat16"):
        for g, sample in w["double_" + name]:
            assert sample in go.WITNESS_SAMPLES
            exact = fr(g) * f(sample)
            by_definition = go.round_fraction(go.round_fraction(exact, "float32"), name)
            assert by_definition != go.round_fraction(exact, name), (name, g, sample)
            # the oracle is on the definition's side
            got = go.gain_expected(_rows([sample]), np.array([g], dtype=np.float32), name)
            assert fr(go.from_bits(got, name).float().item()) == by_definition
    for old, g, sample in w["fused"]:
        exact = fr(g) * f(sample)
        two = go.round_fraction(fr(old) + go.round_fraction(exact, "float32"), "float32")
        assert two != go.round_fraction(fr(old) + exact, "float32"), (old, g, sample)
        assert go.round_fraction(fr(old), "bfloat16") == fr(old)  # a value of every row type
        old_bits = np.array([[[np.float32(old).view(np.uint32)]]], dtype=np.uint32)
        got = go.gain_expected(_rows([sample]), np.array([g], dtype=np.float32), "float32", old_bits)
        assert fr(go.from_bits(got, "float32").item()) == two
    for g, sample in w["order"]:
        assert 2.0 ** -134 <= float(g) < 2.0 ** -133
        once = go.round_fraction(fr(g) * f(sample), "float32")
        twice = go.round_fraction(go.round_fraction(fr(g) * sample, "float32") / 32768, "float32")
        assert once != twice and abs(once) < Fraction(2) ** -126, (g, sample)
        got = go.gain_expected(_rows([sample]), np.array([g], dtype=np.float32), "float32")
        assert fr(go.from_bits(got, "float32").item()) == once


def test_witness_windows_point_at_the_header_samples():
    spb = 100
    windows, gains, olds = go.witness_windows(5, spb)
    w = go.witnesses()
    assert len(windows) == len(gains) == sum(len(v) for v in w.values()) and len(olds) == len(w["fused"])
    assert set(windows[:, 0].tolist()) == {5} and set(windows[:, 1].tolist()) <= {0, spb}
    hist = go.witness_histories()
    for i, t, old in olds:
        sample = hist[windows[i, 1] // spb][t]
        assert (np.float32(old), gains[i], sample) in [(np.float32(o), g, s) for o, g, s in w["fused"]]


# ---- the witnesses on the vector path ----------------------------------------------------------------------------------------------
def _matrix_cases():
    """every case of tests/test_gpu_window_decode_matrix.py, as the GPU file itself builds it (on the CPU, cached)"""
    import test_gpu_window_decode_matrix as gm
    import window_matrix as wm
    keys = [("same", g) for g in wm.GEOMETRIES] + [("mixed", p) for p in wm.MIXED_PLANS] + [("mix", oc) for oc in wm.OUT_CHANNELS]
    return gm, [(k, gm.matrix_case(*k)) for k in keys]


def test_chunk_elements_and_classes_by_hand():
    assert list(go.chunk_elements(150, 225)) == list(range(4, 4 + 16 * 9))   # (150 - 4) // 16 = 9 chunks, the crop is longer
    assert list(go.chunk_elements(150, 40)) == list(range(4, 36))            # (40 - 4) // 16 = 2: the span ends inside the third
    assert list(go.chunk_elements(19, 225)) == [] and list(go.chunk_elements(150, 3)) == []
    assert [int(go.chunk_class(np.int64(t))) for t in (4, 5, 11, 12, 13, 19, 20, 21, 28)] == [0, 1, 1, 2, 3, 3, 0, 1, 2]


def test_vector_witnesses_of_the_matrix_are_witnesses():
    """each witness the matrix cases carry, with fractions.Fraction on the oracle's own row value: never with the code under test"""
    gm, cases = _matrix_cases()
    fr = lambda v: Fraction(float(v))
    total = 0
    for key, case in cases:
        assert len(case.witnesses) == 16 * len(case.variants) > 0
        for i, w in enumerate(case.witnesses):
            k = case.n_plain + i
            stream = int(case.windows[k, 0])
            mono_twin = key[0] == "mix" and case.channels == 2 and case.headers[stream].num_channels == 1
            down = key[0] == "mix" and case.channels == 1 and case.headers[stream].num_channels == 2
            scale = 65536 if down else 32768
            f = fr(case.rows32[k, w.channel, w.t])
            s = f * scale
            assert s.denominator == 1 and 0 < abs(s) <= (65535 if down else 32768), (key, i, f)  # the integer the decoder holds
            g = fr(w.gain)
            assert case.gains[k] == w.gain and fr(np.float32(w.gain)) == g
            exact = g * f
            one = np.array([w.gain], dtype=np.float32)
            row = case.rows32[k:k + 1, w.channel:w.channel + 1, w.t:w.t + 1]
            if w.kind.startswith("double_"):
                name = w.kind[len("double_"):]
                by_definition = go.round_fraction(go.round_fraction(exact, "float32"), name)
                assert by_definition != go.round_fraction(exact, name), (key, i, w)
                assert fr(go.from_bits(go.gain_expected(row, one, name), name).float().item()) == by_definition
                assert w.olds is None
            elif w.kind == "fused":
                rows = [r for r, _ in w.olds]
                assert rows == ([0, 1] if mono_twin else [w.channel]), (key, i, w)
                assert len({old for _, old in w.olds}) == len(w.olds)  # twin rows: two different old values
                for r, old in w.olds:
                    assert case.rows32[k, r, w.t] == case.rows32[k, w.channel, w.t]
                    assert go.round_fraction(fr(old), "bfloat16") == fr(old)  # a value of every row type
                    two = go.round_fraction(fr(old) + go.round_fraction(exact, "float32"), "float32")
                    assert two != go.round_fraction(fr(old) + exact, "float32"), (key, i, w)
                    old_bits = np.array([[[np.float32(old).view(np.uint32)]]], dtype=np.uint32)
                    assert fr(go.from_bits(go.gain_expected(row, one, "float32", old_bits), "float32").item()) == two
                    assert (k, r, w.t, old) in case.olds
            else:
                assert w.kind == "order" and 2.0 ** -134 <= float(w.gain) < 2.0 ** -133 and w.olds is None
                once = go.round_fraction(exact, "float32")
                twice = go.round_fraction(go.round_fraction(g * s, "float32") / scale, "float32")
                assert once != twice and abs(once) < Fraction(2) ** -126, (key, i, w)
                assert fr(go.from_bits(go.gain_expected(row, one, "float32"), "float32").item()) == once
            total += 1
    assert total == 16 * (12 + 3 + 6 + 3 + 9 + 9)


def test_vector_witnesses_cover_the_four_classes_and_rotate_the_channel():
    _, cases = _matrix_cases()
    for key, case in cases:
        by_stream = {}
        for i, w in enumerate(case.witnesses):
            stream = int(case.windows[case.n_plain + i, 0])
            by_stream.setdefault((stream, w.kind), []).append(w)
        assert len(by_stream) == len(go.VECTOR_KINDS) * len(case.variants)
        for (stream, kind), ws in by_stream.items():
            classes = sorted(((w.t - 4) % 2, (w.t - 4) % 16 >= 8) for w in ws)  # the half of the word, the put8 call
            assert classes == [(0, False), (0, True), (1, False), (1, True)], (key, stream, kind, classes)
            assert [int(go.chunk_class(np.int64(w.t))) for w in ws] == [0, 1, 2, 3]
        for stream in {s for s, _ in by_stream}:
            if case.rows32.shape[1] > 1:
                seen = {w.channel for (s, _), ws in by_stream.items() if s == stream for w in ws}
                assert len(seen) == case.rows32.shape[1], (key, stream, seen)


def test_vector_witnesses_lie_on_the_chunk_path():
    """by the formula - t in [4, 4 + 16 m), m = min((spb - 4) // 16, (Le - 4) // 16), the window on a block boundary of a complete
    block - and by a restatement of the lane's own arithmetic: lane k = 0 of the window keeps [lo, hi) = [0, min(spb, Le)),
    decodes n = min(num_samples - first_frame, hi) samples, of them (n - 4) // 16 whole chunks, and chunk t0 goes out by the vector
    stores when whole(t0): t0 >= lo and t0 + 16 <= hi.  Le: T in the gain run, the clipped span in the placed run."""
    gm, cases = _matrix_cases()
    for key, case in cases:
        frames = case.frames
        for i, w in enumerate(case.witnesses):
            k = case.n_plain + i
            stream, first = case.windows[k].tolist()
            spb, header = case.spbs[stream], case.headers[stream]
            block = first // spb
            assert first % spb == 0 and first + spb <= case.lengths[stream]                   # a block boundary, a complete block
            assert 31 + (block + 1) * header.block_size + 18 <= len(case.images[stream])      # ... untruncated, another one behind
            length, o = case.spans[k].tolist()
            assert o == 1 + i % gm.WITNESS_SHIFTS and 0 < o and length == frames - o
            for le in (frames, min(length, frames - o)):
                m = min((spb - 4) // 16, (le - 4) // 16)
                assert m >= 2 and 4 <= w.t < 4 + 16 * m, (key, i, w, le)
                assert w.t in go.chunk_elements(spb, le)
                lo, hi = 0, min(spb, le)
                n = min(case.lengths[stream] - first, hi)
                full = (n - 4) // 16
                t0 = 4 + 16 * ((w.t - 4) // 16)
                assert (t0 - 4) // 16 < full and t0 >= lo and t0 + 16 <= hi, (key, i, w, le)
            assert o + w.t < frames


# ---- snr_gains ---------------------------------------------------------------------------------------------------------------------
def test_snr_gains_against_float64():
    s = torch.tensor([[[4000000, 9, 9, 100], [1000000, 9, 9, 100]],   # stereo: P = 5e6 / 200
                      [[250000, 9, 9, 50], [0, 0, 0, 50]],
                      [[0, 0, 0, 10], [0, 0, 0, 10]],               # silent signal
                      [[77, 9, 9, 0], [5, 9, 9, 0]],                # no frames
                      [[123456789012, 9, 9, 333], [98765, 9, 9, 333]]], dtype=torch.int64)
    n = torch.tensor([[[10000, 9, 9, 100]], [[400, 9, 9, 25]], [[500, 9, 9, 10]], [[500, 9, 9, 10]], [[0, 0, 0, 333]]], dtype=torch.int64)  # mono
    got = snr_gains(s, n, 10.0)
    assert got.dtype == torch.float32 and got.shape == (5,)
    want = []
    for i in range(5):
        ps_sum, pc = int(s[i, :, 0].sum()), int(s[i, :, 3].sum())
        ns_sum, nc = int(n[i, :, 0].sum()), int(n[i, :, 3].sum())
        if 0 in (ps_sum, pc, ns_sum, nc):
            want.append(0.0)
        else:
            want.append(math.sqrt((ps_sum / pc) / (ns_sum / nc)) * 10.0 ** (-10.0 / 20.0))
    assert want[0] > 0 and want[1] > 0 and want[2:] == [0.0, 0.0, 0.0]
    assert np.allclose(got.numpy().astype(np.float64), np.array(want), rtol=2.0 ** -23, atol=0.0)
    per_window = snr_gains(s, n, torch.tensor([10.0, 0.0, 3.0, 3.0, 3.0]))
    assert per_window[0] == got[0] and np.isclose(float(per_window[1]), want[1] * 10.0 ** 0.5, rtol=2.0 ** -23)
    # the other way round: a stereo noise under a mono signal
    back = snr_gains(n, s, -10.0)
    assert np.isclose(float(back[0]) * want[0], 1.0, rtol=2.0 ** -22) and float(back[4]) == 0.0
    with pytest.raises(ValueError):
        snr_gains(s.to(torch.int32), n, 0.0)


# ---- the engine's refusals ---------------------------------------------------------------------------------------------------------
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


def test_a_run_with_neither_argument_is_the_plain_call(engine):
    plan, good = _plan(engine)
    plan.run(good["data"], good["windows"], FRAMES)
    plan.run(good["data"], good["windows"], FRAMES, gain=None, accumulate=False)
    assert [c[0] for c in engine.lib.runs()] == ["AADHip_WindowDecodePlanRun"] * 2
    assert len(engine.lib.last("AADHip_WindowDecodePlanRun")) == 7


def test_gain_runs_hand_over_the_table_and_the_mode(engine):
    plan, good = _plan(engine)
    gain = torch.ones(W)
    out = plan.run(good["data"], good["windows"], FRAMES, torch.float16, gain=gain)
    assert out.dtype == torch.float16 and out.shape == (W, CH, FRAMES)
    args = engine.lib.last("AADHip_WindowDecodePlanRunGain")
    assert args[1:] == (good["data"].data_ptr(), W, good["windows"].data_ptr(), FRAMES, capi.SAMPLE_FLOAT16, out.data_ptr(), gain.data_ptr(), 0)
    assert plan.run(good["data"], good["windows"], FRAMES, torch.float16, out=out, accumulate=True) is out
    assert engine.lib.last("AADHip_WindowDecodePlanRunGain")[-3:] == (out.data_ptr(), None, 1)
    plan.run(good["data"], good["windows"], FRAMES, out=torch.zeros((W, CH, FRAMES)), gain=gain, accumulate=True)
    assert engine.lib.last("AADHip_WindowDecodePlanRunGain")[-2:] == (gain.data_ptr(), 1)
    assert [c[0] for c in engine.lib.runs()] == ["AADHip_WindowDecodePlanRunGain"] * 3


def test_refusals_reach_no_run(engine):
    plan, good = _plan(engine)
    run = lambda **kw: plan.run(good["data"], good["windows"], FRAMES, **kw)
    gain = torch.ones(W)
    with pytest.raises(ValueError, match="int16"):
        run(dtype=torch.int16, gain=gain)
    with pytest.raises(ValueError, match="int16"):
        run(dtype=torch.int16, out=torch.zeros((W, CH, FRAMES), dtype=torch.int16), accumulate=True)
    with pytest.raises(ValueError, match="`out`"):
        run(accumulate=True)
    with pytest.raises(ValueError, match="statistics-only run"):
        run(gain=gain, stats=True)
    with pytest.raises(ValueError, match="statistics-only run"):
        run(out=torch.zeros((W, CH, FRAMES)), accumulate=True, stats=torch.zeros((W, CH, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="statistics-only run"):
        run(gain=gain, stats=True, rows=False)
    with pytest.raises(ValueError, match="gain: dtype torch.float32"):
        run(gain=gain.double())
    with pytest.raises(ValueError, match="gain: shape"):
        run(gain=torch.ones(W + 1))
    with pytest.raises(ValueError, match="gain: shape"):
        run(gain=torch.ones((W, 1)))
    with pytest.raises(ValueError, match="gain: a tensor on the engine's device"):
        run(gain=torch.empty(W, device="meta"))
    with pytest.raises(ValueError, match="gain: a contiguous tensor"):
        run(gain=torch.ones(2 * W)[::2])
    with pytest.raises(ValueError, match="gain: a contiguous tensor"):
        plan.run(good["data"], good["windows"], FRAMES, gain=torch.ones(2 * W)[::2], ordered=False)
    with pytest.raises(ValueError, match="gain: a torch tensor"):
        run(gain=[1.0] * W)
    assert engine.lib.runs() == []
