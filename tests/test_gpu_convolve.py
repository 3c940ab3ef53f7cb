"""Reverberation on the device (AADHip_ConvolverResolve -> AADHip_WindowDecodePlanRun -> AADHip_ConvolverRun / ...RunGain,
aad_amd/csrc/aad_convolve.hip): crops of a corpus convolved with a per-window impulse response into planar [N, C, T] rows, the
sums as int8 matrix products.

Bar: bit for bit against the definition (include/aad_hip.h "reverberation", restated in tests/convolve_oracle.py over the
library's own taps, which tests/test_convolve_host.py holds to the oracle's quantiser), canaries on both sides of every buffer.
  * the corpora of tests/test_gpu_window_resample.py - the three kinds of window decode plan - at T = 257 and T = 1025, all four
    sample types, responses of K = 1, 2, 16, 17, 63, 64, 65, 128, 1000, 4096 and 32768 taps (every length where a k-step, a
    fragment or a staged piece begins or ends) with scales from q = 0 to 15 and the delays 0, K - 1 and the default; windows below,
    at and above each response's lead, across and past the stream's end, wrapped and huge, stray streams, stray and negative
    response indices, a NULL response table;
  * the {1.0} response equal to Engine.decode_windows_mixed, byte for byte, for the four types;
  * hand-made source rows through run_source: every tap +32639 and every tap -32639 over rows on both rails at K = 4096 and 32768
    (an int32-wrapped sum and a float32-accumulated sum give other bits, asserted on the CPU first); taps with a low byte of -128
    and high bytes of +-127 over a row that is zero but for one frame (the padding's low byte -128 goes through the constant
    128 sum h); the float32 ties 2^24 + 1 and 2^24 + 3; a ramp times an alternating sign, which a swapped or mirrored fragment
    map cannot pass;
  * gain: three float types x STORE / ADD, gains 1, -1, 0, 1e-41, random and crafted ones - a fused multiply-add and a 2-byte
    pack without the float32 rounding give other bits, asserted on the CPU first (tests/resample_mix_oracle.py, the responses
    at Q = 14 so that its scale 2^-29 is this stage's); the span list of tests/test_gpu_resample_mix.py, STORE into NaNs, ADD over
    NaNs and -0; NULL spans, NULL gain and STORE equal to the plain run;
  * T = 10757 - two full tiles of 4096 outputs and a tail of eleven blocks, so that waves keep four, three and two blocks - with
    responses past one staged piece, two channel rows a window, plain in the four types and through the gain kernels with spans
    across elements 4096 and 8192, ending before the second tile and starting behind the first;
  * one grid past 2^20 workgroups (T = 1, K = 1: the item loop);
  * the C calls' refusals, each once, which leave canaries untouched, and the Python level's."""
import numpy as np
import pytest

import convolve_oracle as co
import resample_mix_oracle as mo
import window_gain_oracle as go
import window_placed_oracle as po
from aad_amd.capi import (AADApiResult, SAMPLE_BFLOAT16, SAMPLE_FLOAT16, SAMPLE_FLOAT32, SAMPLE_INT16, WINDOW_GAIN_ADD,
                          WINDOW_GAIN_STORE)
from aad_amd.engine import ConvolveSource
from test_gpu_resample_mix import CANARY, MINUS_ZERO, NAN, Bordered, _direct, _host, _random_old, _spans
from test_gpu_window_resample import CASES, DTYPES, FRAMES, LENGTHS, _bits, _compare, corpora, engine  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = {"int16": SAMPLE_INT16, "float32": SAMPLE_FLOAT32, "float16": SAMPLE_FLOAT16, "bfloat16": SAMPLE_BFLOAT16}
CASE_IDS = ["same_format", "mixed_format", "channel_mix_mono", "channel_mix_stereo"]
TAPS = [65, 1, 2, 16, 17, 63, 64, 128, 1000, 4096, 32768]
_CACHE = {}


def _responses(rotate, unit_peak):
    """float32 responses of the lengths TAPS: a peak and a decaying tail.  unit_peak: the peak is 1.0 and every response has
    Q = 14; else the scales run from q = 0 to 15.  Delays: the default, 0 and K - 1 in turn, turned by `rotate`."""
    rng = np.random.default_rng(40 + rotate)
    hs, delays = [], []
    for i, K in enumerate(TAPS):
        h = rng.uniform(-0.9, 0.9, size=K) * np.exp(-np.arange(K) * (6.0 / K))
        h[(K // 3) if i % 2 else 0] = 1.0
        if not unit_peak:
            h *= (1.0, 0.3, 3.0, 20000.0, 200.0)[i % 5]
        hs.append(h.astype(np.float32))
        delays.append((None, 0, K - 1)[(i + rotate) % 3])
    return hs, delays


def _windows(responses):
    """windows and response indices: per response the edges of its own lead, then the strays"""
    rows, index = [], []
    R = len(responses)
    for r, (taps, _, d) in enumerate(responses):
        K = len(taps)
        lead = K - 1 - d
        s = 1 + r % 2  # the two streams of 3000 frames
        n = LENGTHS[s]
        firsts = [max(lead - 1, 0), lead, lead + 1, [0, 1234, n - 100, n - 1, n, n + K][r % 6]]
        rows += [(s, f) for f in firsts]
        index += [r] * len(firsts)
    rows += [(0, 650), (3, 0), (3, 39), (3, 40)]  # short streams
    index += [0, 8, 9, 10]
    strays = [((len(LENGTHS), 5), 0), ((-1, 5), 0), (((1 << 63) - 1, 0), 1),      # no such stream
              ((1, 5), R), ((1, 5), -1), ((1, 5), 1 << 40), ((1, 5), -(1 << 63)),   # no such response
              ((1, -1), 1), ((2, 1 << 40), 2), ((2, -(1 << 62)), 9), ((1, (1 << 63) - 1), 10)]  # wrapped and huge starts
    rows += [s[0] for s in strays]
    index += [s[1] for s in strays]
    return np.array(rows, dtype=np.int64), np.array(index, dtype=np.int64)


def _expected(decoded, windows, index, responses, frames, channels):
    """-> (int64 acc [N, channels, frames], zeros for a window without a stream or a response; q per window)"""
    acc = np.zeros((len(windows), channels, frames), dtype=np.int64)
    qs = np.zeros(len(windows), dtype=np.int64)
    for w, (s, f) in enumerate(windows.tolist()):
        r = 0 if index is None else int(index[w])
        if not (0 <= s < len(decoded)) or not (0 <= r < len(responses)):
            continue
        qs[w] = responses[r][1]
        for c in range(channels):
            acc[w, c] = co.row(decoded[s][:, c], len(decoded[s]), f, frames, responses[r])
    return acc, qs


def _convert(acc, qs, name):
    out = np.stack([co.element_bits(acc[w], int(qs[w]), name) for w in range(len(acc))])
    return out.view(np.int16) if name == "int16" else out


def _float_rows(acc, qs):
    return np.stack([co.to_float32(acc[w], int(qs[w])) for w in range(len(acc))])


class Setup:
    """one case at one T: plan, convolver, windows, the decoded source batch and the oracle's acc, shared by the tests"""

    def __init__(self, engine, corpora, case_index, frames, unit_peak):  # noqa: F811
        import torch
        name, channels = CASES[case_index]
        images, data, table, headers, rows = corpora[name]
        self.channels, self.frames = channels, frames
        self.d_img = torch.from_numpy(data).cuda()
        if name == "same":
            self.plan = engine.window_decode_plan(headers[0], table)
        elif name == "mixed":
            self.plan = engine.mixed_window_decode_plan(headers, table)
        else:
            self.plan = engine.channel_mix_window_decode_plan(headers, table, channels)
        hs, delays = _responses(case_index, unit_peak)
        self.conv = engine.convolver(hs, delays)
        self.responses = []
        for r, (h, d) in enumerate(zip(hs, delays)):
            q, delay, taps = self.conv.response(r)
            want = co.quantise(h, d)
            assert (q, delay) == want[1:] and np.array_equal(taps, want[0]) and (d is None or d == delay), r
            self.responses.append((taps.astype(np.int64), q, delay))
        self.windows, self.index = _windows(self.responses)
        self.n = len(self.windows)
        key = (name, channels, frames, unit_peak)
        if key not in _CACHE:
            _CACHE[key] = _expected(rows[channels], self.windows, self.index, self.responses, frames, channels)
        self.acc, self.qs = _CACHE[key]
        self.variant = self.index  # _compare's label
        self.d_windows = torch.from_numpy(self.windows).cuda()
        self.d_index = torch.from_numpy(self.index).cuda()
        self.decoded = rows[channels]

    def close(self):
        self.conv.close()
        self.plan.close()


PARAMS = [(c, f) for c in range(len(CASES)) for f in FRAMES]
PARAM_IDS = ["%s-%d" % (CASE_IDS[c], f) for c, f in PARAMS]


@pytest.fixture(params=PARAMS, ids=PARAM_IDS)
def setup(request, engine, corpora):  # noqa: F811
    s = Setup(engine, corpora, request.param[0], request.param[1], False)
    yield s
    s.close()


@pytest.fixture(params=PARAMS, ids=PARAM_IDS)
def unit_setup(request, engine, corpora):  # noqa: F811
    s = Setup(engine, corpora, request.param[0], request.param[1], True)
    s.source = s.conv.decode_source(s.plan, s.d_img, s.d_windows, s.frames, response=s.d_index)
    yield s
    s.close()


# ---- plain rows ----------------------------------------------------------------------------------------------------------------------
def test_rows_equal_the_definition(engine, setup):  # noqa: F811
    import torch
    s = setup
    shape = (s.n, s.channels, s.frames)
    assert sorted({q for _, q, _ in s.responses})[0] == 0 and 15 in {q for _, q, _ in s.responses}
    assert s.conv.source_frames(s.frames) == co.source_frames(s.frames, s.responses) == s.frames + 32767
    assert (s.acc != 0).any(axis=(1, 2)).sum() > s.n // 2
    assert (np.abs(s.acc) > 1 << 31).any()  # sums that int32 does not hold
    for name in DTYPES:
        out = Bordered(torch, shape, name, CANARY[name])
        got = s.conv.run(s.plan, s.d_img, s.d_windows, s.frames, response=s.d_index, dtype=getattr(torch, name), out=out.view)
        assert got.data_ptr() == out.view.data_ptr()
        _compare(out.bits(), _convert(s.acc, s.qs, name), (name,), s.windows, s.index)
    # no response table: every window takes response 0
    acc0, q0 = _expected(s.decoded, s.windows, None, s.responses, s.frames, s.channels)
    out = Bordered(torch, shape, "int16", CANARY["int16"])
    s.conv.run(s.plan, s.d_img, s.d_windows, s.frames, dtype=torch.int16, out=out.view)
    _compare(out.bits(), _convert(acc0, q0, "int16"), ("no responses",), s.windows, None)


def test_the_unit_response_equals_decode_windows_mixed(engine, corpora):  # noqa: F811
    import torch
    images, data, table, headers, rows = corpora["mixed"]
    d_img = torch.from_numpy(data).cuda()
    sizes = [len(i) for i in images]
    windows = np.array([(0, 0), (1, 5), (2, 2990), (3, 39), (3, 40), (1, 3000), (4, 0), (-1, 3), (2, -1), (0, 1 << 40)], dtype=np.int64)
    d_win = torch.from_numpy(windows).cuda()
    for frames in FRAMES:
        for name in DTYPES:
            dtype = getattr(torch, name)
            want = engine.decode_windows_mixed(d_img, sizes, d_win, frames, dtype)
            got = engine.decode_windows_reverberated(d_img, sizes, d_win, frames, [[1.0]], dtype=dtype)
            assert got.dtype == dtype and got.shape == want.shape
            assert _bits(torch, got).tobytes() == _bits(torch, want).tobytes(), (frames, name)


# ---- hand-made source rows -----------------------------------------------------------------------------------------------------------
def _run_rows(engine, conv, rows, lanes, frames, name):  # noqa: F811
    """hand-made int16 rows [N, C, T_src] and lanes through run_source into a bordered buffer -> the rows' bits"""
    import torch
    n, ch, t_src = rows.shape
    src = Bordered(torch, rows.shape, "int16", rows.view(np.uint16))
    out = Bordered(torch, (n, ch, frames), name, CANARY[name])
    conv.run_source(ConvolveSource(src.view, torch.from_numpy(lanes).cuda(), t_src), frames, ch, getattr(torch, name), out=out.view)
    return out.bits()


def _hand_acc(rows, lanes, frames, responses):
    """-> (int64 acc [N, C, frames], q per row): the source row's element `shift` holds the window's first frame"""
    acc = np.zeros(rows.shape[:2] + (frames,), dtype=np.int64)
    qs = np.zeros(len(rows), dtype=np.int64)
    for w in range(len(rows)):
        taps, qs[w], d = responses[int(lanes[w, 0])]
        for c in range(rows.shape[1]):
            acc[w, c] = co.sums(rows[w, c], int(lanes[w, 1]), frames, taps, d)
    return acc, qs


@pytest.mark.parametrize("K", [4096, 32768])
def test_full_scale_taps_over_rows_on_both_rails(engine, K):  # noqa: F811
    frames = 257
    conv = engine.convolver([np.full(K, 32639.0), np.full(K, -32639.0)], delays=[K - 1, 0])
    try:
        responses = [(t.astype(np.int64), q, d) for q, d, t in (conv.response(0), conv.response(1))]
        assert [r[1:] for r in responses] == [(0, K - 1), (0, 0)] and (responses[0][0] == 32639).all() and (responses[1][0] == -32639).all()
        t_src = conv.source_frames(frames)
        rng = np.random.default_rng(K)
        rows = np.zeros((6, 1, t_src), dtype=np.int16)
        rows[0], rows[1], rows[2] = 32767, -32768, 32767
        rows[3], rows[4] = -32768, np.where(rng.integers(0, 2, size=t_src) == 1, 32767, -32768)
        rows[5] = rng.integers(-32768, 32768, size=t_src)
        lanes = np.array([[0, 0], [0, 0], [1, K - 1], [1, K - 1], [0, 0], [1, K - 1]], dtype=np.int32)
        acc, qs = _hand_acc(rows, lanes, frames, responses)
        for rail in (32767 * 32639 * K, -32768 * 32639 * K, 32768 * 32639 * K, -32767 * 32639 * K):  # both rails under every tap
            assert (acc == rail).any(), rail
        # other arithmetic gives other bits among the compared elements: a sum that wraps at 32 bits, and one accumulated in float32
        right = co.element_bits(acc[:, 0], 0, "float32")
        assert (co.element_bits(acc[:, 0].astype(np.int32).astype(np.int64), 0, "float32") != right).any()
        in_float = []
        for w in range(6):  # element 0 of every row, its K products added one by one in float32
            taps, _, d = responses[lanes[w, 0]]
            x = rows[w, 0, int(lanes[w, 1]) + d - np.arange(K)]
            in_float.append(np.cumsum(taps.astype(np.float32) * x.astype(np.float32), dtype=np.float32)[-1])
        assert ((np.array(in_float, dtype=np.float32) * np.float32(2.0 ** -15)).view(np.uint32) != right[:, 0]).any()
        for name in DTYPES:
            _compare(_run_rows(engine, conv, rows, lanes, frames, name), _convert(acc, qs, name), (K, name), lanes, None)
    finally:
        conv.close()


@pytest.mark.parametrize("frames", FRAMES)
def test_crafted_taps_on_hand_made_rows(engine, frames):  # noqa: F811
    edge = np.array([32639, -128, 128, 32384, -32639, -32512, 127, -127, 0, -1, 1, 255, 256, -256, -255, -129, 0x7E80, -0x7E80], dtype=np.float64)
    ties = np.array([1, 4096, 0, 32639], dtype=np.float64)
    k = np.arange(1000)
    ramp = (k + 1) * np.where(k % 2 == 1, -1.0, 1.0) * 32.0  # asymmetric: no mirror image, no shift of itself
    conv = engine.convolver([edge, ties, ramp, np.tile(edge, 8)[:129]], delays=[0, 0, None, 64])
    try:
        responses = [(t.astype(np.int64), q, d) for q, d, t in (conv.response(r) for r in range(4))]
        assert [r[1] for r in responses] == [0, 0, 0, 0] and responses[0][0].tolist() == edge.astype(np.int64).tolist()
        assert responses[2][2] == 999 and responses[2][0][999] == -32000
        t_src = conv.source_frames(frames)
        rng = np.random.default_rng(frames)
        rows = np.zeros((9, 2, t_src), dtype=np.int16)
        rows[0, 0, 40], rows[0, 1, frames - 1] = 0x1280, -1           # zero but for one frame: the rest is padding bytes (0, -128)
        rows[1, 0, 0], rows[1, 1, t_src - 1] = -32768, 32767
        rows[2, 0, 10:12], rows[2, 0, 200:202] = [4096, 1], [4096, 3]  # acc = 2^24 + 1, 2^24 + 3 under response 1
        rows[2, 1, 10:12], rows[2, 1, 200:202] = [-4096, -1], [-4096, -3]
        rows[3:] = rng.integers(-32768, 32768, size=(6, 2, t_src))
        lanes = np.array([[0, 0], [0, 17], [1, 0], [2, 0], [2, 0], [3, 64], [3, 0], [0, 5], [4, 0]], dtype=np.int32)
        lanes[8, 0] = -1  # 0xFFFFFFFF: no response
        acc_ties = co.sums(rows[2, 0], 0, frames, responses[1][0], 0)
        assert acc_ties[11] == (1 << 24) + 1 and acc_ties[201] == (1 << 24) + 3
        acc, qs = _hand_acc(rows[:8], lanes[:8], frames, responses)
        acc, qs = np.concatenate([acc, np.zeros_like(acc[:1])]), np.concatenate([qs, [0]])  # no response: +0
        for name in DTYPES:
            _compare(_run_rows(engine, conv, rows, lanes, frames, name), _convert(acc, qs, name), (frames, name), lanes, None)
    finally:
        conv.close()


def test_rows_past_the_tile(engine):  # noqa: F811
    """Two full tiles of 4096 outputs and a tail of eleven blocks (waves with four, three and two blocks), two channel rows a
    window, responses past one staged piece of 4096 taps: the plain kernels in the four types and the gain kernels with spans
    that cross elements 4096 and 8192, end before the second tile, start behind the first, or are empty."""
    import torch
    frames = 2 * 4096 + 10 * 256 + 5
    rng = np.random.default_rng(8192)
    hs = [rng.uniform(-0.9, 0.9, size=K) * np.exp(-np.arange(K) * (6.0 / K)) for K in (4200, 97, 4500)]
    hs[0][1400], hs[1][0], hs[2][4499] = 1.0, 0.3, 3.0
    conv = engine.convolver(hs, delays=[None, 0, 4499])
    try:
        responses = [(t.astype(np.int64), q, d) for q, d, t in (conv.response(r) for r in range(3))]
        assert [(r[1], r[2]) for r in responses] == [(14, 1400), (15, 0), (13, 4499)]
        t_src = conv.source_frames(frames)
        assert t_src == frames + 4499
        n, ch = 7, 2
        rows = rng.integers(-32768, 32768, size=(n, ch, t_src)).astype(np.int16)
        lanes = np.array([[0, 4199 - 1400], [1, 96], [2, 0], [0, 0], [1, 0], [2, 0], [3, 0]], dtype=np.int32)
        lanes[6, 0] = -1  # 0xFFFFFFFF: no response
        acc, qs = _hand_acc(rows[:6], lanes[:6], frames, responses)
        acc, qs = np.concatenate([acc, np.zeros_like(acc[:1])]), np.concatenate([qs, [0]])
        assert (np.abs(acc) > 1 << 31).any()
        for name in DTYPES:
            _compare(_run_rows(engine, conv, rows, lanes, frames, name), _convert(acc, qs, name), (frames, name), lanes, None)
        # gain and spans: crop index n lands at row element o + n
        spans = np.array([(frames, 0), (600, 3800), (3000, 500), (5000, 4000), (frames, 4097), (0, 0), (9000, 1)], dtype=np.int64)
        inside = np.zeros((n, ch, frames), dtype=bool)
        for w, (le, o) in enumerate(po.clipped(spans, n, frames)):
            inside[w, :, o:o + le] = True
        assert inside[1, 0, 4095] and inside[1, 0, 4096] and not inside[2, 0, 4096:].any() and inside[3, 0, 8192] and not inside[4, 0, :4097].any()
        gains = np.array([1.0, -1.5, 0.75, 1e-41, -0.3, 2.0, -1.0], dtype=np.float32)
        rows32 = _float_rows(acc, qs)
        src = Bordered(torch, rows.shape, "int16", rows.view(np.uint16))
        source = ConvolveSource(src.view, torch.from_numpy(lanes).cuda(), t_src)
        d_gain, d_spans = torch.from_numpy(gains).cuda(), torch.from_numpy(spans).cuda()
        for name in go.DTYPES:
            store = Bordered(torch, (n, ch, frames), name, NAN[name])  # STORE into NaNs: every element is defined afterwards
            conv.run_source(source, frames, ch, go.torch_dtype(name), out=store.view, gain=d_gain, spans=d_spans)
            want = po.placed_expected(rows32, spans, gains, name)
            assert not (want == NAN[name]).any() and not (want[~inside] != 0).any()
            _compare(store.bits(), want, ("STORE", name), lanes, None)
            old = _random_old(rng, (n, ch, frames), name)  # ADD: NaNs and -0 outside the spans keep their bits
            outside = np.where(rng.integers(0, 2, size=old.shape) == 1, NAN[name], MINUS_ZERO[name]).astype(old.dtype)
            old[~inside] = outside[~inside]
            add = Bordered(torch, (n, ch, frames), name, old)
            conv.run_source(source, frames, ch, go.torch_dtype(name), out=add.view, gain=d_gain, accumulate=True, spans=d_spans)
            want = po.placed_expected(rows32, spans, gains, name, old)
            assert (want[~inside] == old[~inside]).all()
            _compare(add.bits(), want, ("ADD", name), lanes, None)
            full = Bordered(torch, (n, ch, frames), name, NAN[name])  # no spans: the whole rows through the gain kernel
            conv.run_source(source, frames, ch, go.torch_dtype(name), out=full.view, gain=d_gain)
            _compare(full.bits(), po.placed_expected(rows32, None, gains, name), ("STORE, no spans", name), lanes, None)
    finally:
        conv.close()


def test_a_grid_past_the_item_loop_threshold(engine):  # noqa: F811
    import torch
    n = (1 << 20) + 77  # T = 1: one item a row
    conv = engine.convolver([[1.0]])
    try:
        rows = np.random.default_rng(3).integers(-32768, 32768, size=(n, 1, 1)).astype(np.int16)
        lanes = np.zeros((n, 2), dtype=np.int32)
        src = Bordered(torch, rows.shape, "int16", rows.view(np.uint16))
        for name in ("int16", "float32"):
            out = Bordered(torch, (n, 1, 1), name, CANARY[name])
            conv.run_source(ConvolveSource(src.view, torch.from_numpy(lanes).cuda(), 1), 1, 1, getattr(torch, name), out=out.view)
            want = co.element_bits(rows.astype(np.int64) * 16384, 14, name)
            assert np.array_equal(out.bits(), want.view(np.int16) if name == "int16" else want), name
    finally:
        conv.close()


# ---- gain and spans --------------------------------------------------------------------------------------------------------------------
def _gains_with_witnesses(s, seed):
    """tests/test_gpu_resample_mix.py's gains over this stage's acc: every response here has Q = 14, the oracle's scale 2^-29"""
    rng = np.random.default_rng(seed)
    gains = rng.uniform(-2.0, 2.0, size=s.n).astype(np.float32)
    inexact = (s.acc.astype(np.float32).astype(np.int64) != s.acc).sum(axis=(1, 2))
    loud = np.argsort(-inexact, kind="stable")[:6].tolist()
    assert inexact[loud[5]] > 16
    quiet = [w for w in range(s.n) if w not in loud and s.acc[w].any()]
    for w, g in zip(quiet, (1.0, -1.0, 0.0, 1e-41)):
        gains[w] = g
    silent = [w for w in range(s.n) if not s.acc[w].any()]
    gains[silent[0]], gains[silent[1]] = -1.5, 1e-41  # -0 rows, and +0 ones
    planted = {name: [] for name in go.DTYPES}
    jobs = [(kind, name) for name in go.DTYPES for kind in ("fused", "double") if (kind, name) != ("double", "float32")]
    for w, (kind, name) in zip(loud, jobs):
        i, g, old = mo.craft(kind, name, s.acc[w].reshape(-1), seed)
        gains[w] = g
        if old is not None:
            planted[name].append((w, i // s.frames, i % s.frames, old))
    return gains, planted


def test_rows_with_gain_store_and_add(engine, unit_setup):  # noqa: F811
    import torch
    s = unit_setup
    assert all(q == 14 for _, q, _ in s.responses)
    rows32 = _float_rows(s.acc, np.full(s.n, 14))
    shape = (s.n, s.channels, s.frames)
    gains, planted = _gains_with_witnesses(s, 31)
    d_gain = torch.from_numpy(gains).cuda()
    rng = np.random.default_rng(77)
    for name in go.DTYPES:
        old = _random_old(rng, shape, name)
        for w, c, t, value in planted[name]:
            old[w, c, t] = go.bits_of(torch.tensor([value], dtype=torch.float32).to(go.torch_dtype(name)))[0]
        # a condition on the inputs: a fused multiply-add and a pack without the float32 rounding are caught by some element
        found = dict(mo.witnesses(s.acc, gains, name), **mo.witnesses(s.acc, gains, name, old))
        assert found["fused"].any() and (name == "float32" or found["double"].any()), name
        store = Bordered(torch, shape, name, CANARY[name])
        got = s.conv.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=store.view, gain=d_gain)
        assert got.data_ptr() == store.view.data_ptr()
        want = po.placed_expected(rows32, None, gains, name)
        assert (want == MINUS_ZERO[name]).any()  # a negative gain on zeros
        _compare(store.bits(), want, ("STORE", name), s.windows, s.index)
        add = Bordered(torch, shape, name, old)
        s.conv.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=add.view, gain=d_gain, accumulate=True)
        _compare(add.bits(), po.placed_expected(rows32, None, gains, name, old), ("ADD", name), s.windows, s.index)


def test_rows_with_spans(engine, unit_setup):  # noqa: F811
    import torch
    s = unit_setup
    rows32 = _float_rows(s.acc, np.full(s.n, 14))
    shape = (s.n, s.channels, s.frames)
    spans = _spans(s.n, s.frames)
    d_spans = torch.from_numpy(spans).cuda()
    rng = np.random.default_rng(5)
    gains = rng.uniform(-2.0, 2.0, size=s.n).astype(np.float32)
    d_gain = torch.from_numpy(gains).cuda()
    inside = np.zeros(shape, dtype=bool)
    for w, (le, o) in enumerate(po.clipped(spans, s.n, s.frames)):
        inside[w, :, o:o + le] = True
    assert inside.any() and not inside.all()
    for name in go.DTYPES:
        store = Bordered(torch, shape, name, NAN[name])  # STORE into NaNs: every element is defined afterwards
        s.conv.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=store.view, gain=d_gain, spans=d_spans)
        want = po.placed_expected(rows32, spans, gains, name)
        assert not (want == NAN[name]).any() and not (want[~inside] != 0).any()
        _compare(store.bits(), want, ("STORE", name), s.windows, s.index)
        old = _random_old(rng, shape, name)  # ADD: NaNs and -0 outside the spans keep their bits
        outside = np.where(rng.integers(0, 2, size=shape) == 1, NAN[name], MINUS_ZERO[name]).astype(old.dtype)
        old[~inside] = outside[~inside]
        add = Bordered(torch, shape, name, old)
        s.conv.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=add.view, gain=d_gain, accumulate=True, spans=d_spans)
        want = po.placed_expected(rows32, spans, gains, name, old)
        assert (want[~inside] == old[~inside]).all()
        _compare(add.bits(), want, ("ADD", name), s.windows, s.index)
    store = Bordered(torch, shape, "float32", NAN["float32"])  # spans without a gain table: every gain is 1
    s.conv.run_source(s.source, s.frames, s.channels, torch.float32, out=store.view, spans=d_spans)
    _compare(store.bits(), po.placed_expected(rows32, spans, None, "float32"), ("STORE", "no gains"), s.windows, s.index)


def test_null_spans_null_gain_store_is_the_plain_run(engine, unit_setup):  # noqa: F811
    import torch
    s = unit_setup
    src = s.source
    for name in go.DTYPES:
        plain = s.conv.run(s.plan, s.d_img, s.d_windows, s.frames, response=s.d_index, dtype=go.torch_dtype(name))
        out = Bordered(torch, (s.n, s.channels, s.frames), name, NAN[name])
        rc = _direct(engine, engine.lib.AADHip_ConvolverRunGain, s.conv.handle, s.n, s.channels, src.rows.data_ptr(), src.source_frames,
                     src.lanes.data_ptr(), None, s.frames, KINDS[name], out.view.data_ptr(), None, WINDOW_GAIN_STORE)
        assert rc == AADApiResult.OK
        assert out.bits().tobytes() == _host(torch, plain, name).tobytes(), name
        assert np.array_equal(out.bits(), _convert(s.acc, s.qs, name))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_c_calls_refuse_and_write_nothing(engine):  # noqa: F811
    import torch
    lib = engine.lib
    n, ch, frames = 3, 2, 40
    conv = engine.convolver([[1.0], np.ones(9)])
    try:
        t_src = conv.source_frames(frames)
        assert t_src == frames + 8
        src = Bordered(torch, (n, ch, t_src), "int16", 7)
        out = Bordered(torch, (n, ch, frames), "float32", CANARY["float32"])
        lanes = torch.zeros((n + 1, 2), dtype=torch.int32, device="cuda")
        windows = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
        source_windows = Bordered(torch, (n, 2), "int64", CANARY["int64"])
        lane_out = Bordered(torch, (n, 4), "int16", CANARY["int16"])
        gain = torch.ones(n + 1, dtype=torch.float32, device="cuda")
        spans = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
        h, S, L, O = conv.handle, src.view.data_ptr(), lanes.data_ptr(), out.view.data_ptr()
        bad = AADApiResult.INVALID_ARGUMENT
        run = lambda *a: _direct(engine, lib.AADHip_ConvolverRun, *a)
        gained = lambda *a: _direct(engine, lib.AADHip_ConvolverRunGain, *a)
        resolve = lambda *a: _direct(engine, lib.AADHip_ConvolverResolve, *a)
        F32 = SAMPLE_FLOAT32
        assert run(h, n, ch, None, t_src, L, frames, F32, O) == bad           # null pointers
        assert run(h, n, ch, S, t_src, None, frames, F32, O) == bad
        assert run(h, n, ch, S, t_src, L, frames, F32, None) == bad
        assert run(h, n, ch, S + 1, t_src, L, frames, F32, O) == bad          # misaligned tables
        assert run(h, n, ch, S, t_src, L + 2, frames, F32, O) == bad
        assert run(h, n, ch, S, t_src, L, frames, F32, O + 2) == bad
        assert run(h, n, ch, S, t_src, L, frames, SAMPLE_FLOAT16, O + 1) == bad
        assert run(h, n, ch, S, t_src, L, 0, F32, O) == bad                   # frames == 0
        assert run(h, n, 0, S, t_src, L, frames, F32, O) == bad               # channels == 0
        assert run(h, n, ch, S, t_src - 1, L, frames, F32, O) == bad          # source rows below T_src
        assert run(h, n, ch, S, t_src, L, frames, 2, O) == bad                # an unknown sample type
        assert run(h, 1 << 62, 4, S, t_src, L, frames, F32, O) == bad         # extents past 64 bits
        assert run(h, 1 << 61, 1, S, t_src, L, frames, F32, O) == bad
        assert gained(h, n, ch, S, t_src, L, None, frames, SAMPLE_INT16, O, None, WINDOW_GAIN_STORE) == bad  # int16 with a gain
        assert gained(h, n, ch, S, t_src, L, spans.data_ptr(), frames, SAMPLE_INT16, O, None, WINDOW_GAIN_ADD) == bad
        assert gained(h, n, ch, S, t_src, L, None, frames, F32, O, None, 2) == bad                            # no such mode
        assert gained(h, n, ch, S, t_src, L, None, frames, F32, O, gain.data_ptr() + 2, WINDOW_GAIN_STORE) == bad
        assert gained(h, n, ch, S, t_src, L, spans.data_ptr() + 4, frames, F32, O, None, WINDOW_GAIN_STORE) == bad
        assert gained(h, n, ch, S, t_src - 1, L, None, frames, F32, O, None, WINDOW_GAIN_STORE) == bad
        W, SW, LO = windows.data_ptr(), source_windows.view.data_ptr(), lane_out.view.data_ptr()
        assert resolve(h, n, None, None, frames, SW, LO) == bad
        assert resolve(h, n, W, None, frames, None, LO) == bad
        assert resolve(h, n, W, None, frames, SW, None) == bad
        assert resolve(h, n, W + 4, None, frames, SW, LO) == bad
        assert resolve(h, n, W, W + 4, frames, SW, LO) == bad
        assert resolve(h, n, W, None, frames, SW, LO + 2) == bad
        assert resolve(h, n, W, None, 0, SW, LO) == bad
        # no windows: OK, and nothing is launched
        assert run(h, 0, ch, S, t_src, L, frames, F32, O) == AADApiResult.OK
        assert gained(h, 0, ch, S, t_src, L, None, frames, F32, O, None, WINDOW_GAIN_ADD) == AADApiResult.OK
        assert resolve(h, 0, W, None, frames, SW, LO) == AADApiResult.OK
        assert (out.bits() == CANARY["float32"]).all() and (source_windows.bits() == CANARY["int64"]).all()
        assert (lane_out.bits().view(np.uint16) == CANARY["int16"]).all()
        # the Python level, before any library call
        with pytest.raises(ValueError, match="out: dtype"):
            conv.run_source(ConvolveSource(src.view, lanes[:n], t_src), frames, ch, torch.float16, out=out.view)
        with pytest.raises(ValueError, match="source.rows: shape"):
            conv.run_source(ConvolveSource(src.view, lanes, t_src), frames, ch)
        with pytest.raises(ValueError, match="float rows only"):
            conv.run_source(ConvolveSource(src.view, lanes[:n], t_src), frames, ch, torch.int16, gain=gain[:n])
        assert (out.bits() == CANARY["float32"]).all()
        # and the good call, after all of them
        ok = conv.run_source(ConvolveSource(src.view, lanes[:n], t_src), frames, ch, out=out.view)
        assert (ok.cpu().numpy() == np.float32(7 / 32768)).all()
    finally:
        conv.close()
