"""Resampled rows with a gain, spans and level statistics on the device (AADHip_ResamplerRunGain, AADHip_ResamplerRunStats;
aad_amd/csrc/aad_resample.hip: resample_rows_gain_kernel, resample_rows_stats_kernel) and Engine.mix_windows_resampled on top.

Bar: bit for bit against tests/resample_mix_oracle.py, with canaries on both sides of every buffer, over the corpora, the ten
ratios and the window list of tests/test_gpu_window_resample.py at T = 257 and T = 1025 (one output past the 1024-output tile):
  * gain: three plan kinds x three float types x STORE / ADD, ADD over random old contents with -0 among them; gains 1, -1, 0, 1e-41
    (subnormal products) and random ones, and on eight loud windows gains (and old values) crafted so that a fused multiply-add,
    a 2-byte pack that skips the float32 rounding and a multiply by the exact acc each give other bits - asserted on the CPU
    before the device is asked;
  * spans: (T, 0), (0, 0), (5, 0), (T, 1) clipped, (10, T - 1), (10, T), (10, 2^40), (-1, 3), an odd and an even offset and at
    T = 1025 (600, 700) across element 1024; STORE into NaNs, ADD over NaNs and -0 outside the spans;
  * NULL spans, NULL gain and STORE equal the plain run;
  * statistics: records with and without spans, with rows (four sample types) and without, `count` against the brute force over
    num_samples, all-zero records without a bank, two runs alike, a pre-filled table overwritten;
  * the C calls on hand-made source rows (the -32768 rail, a +-32767 square wave that clamps), lanes and source statistics;
  * Engine.mix_windows_resampled over 16 kHz and 48 kHz headers to 16 kHz at speeds 1 and 11/10;
  * the C calls' refusals, which leave canaries untouched."""
import numpy as np
import pytest

import oracle_binding as ob
import resample_mix_oracle as mo
import resample_oracle as ro
import window_gain_oracle as go
import window_placed_oracle as po
from aad_amd.capi import (AADApiResult, SAMPLE_BFLOAT16, SAMPLE_FLOAT16, SAMPLE_FLOAT32, SAMPLE_INT16, WINDOW_GAIN_ADD,
                          WINDOW_GAIN_STORE)
from aad_amd.engine import snr_gains
from test_gpu_window_resample import (CASES, DTYPES, FRAMES, LENGTHS, RATIOS, _banks, _compare, _encode, _rows, _windows, corpora,  # noqa: F401
                                      engine)

pytestmark = pytest.mark.gpu

KINDS = {"int16": SAMPLE_INT16, "float32": SAMPLE_FLOAT32, "float16": SAMPLE_FLOAT16, "bfloat16": SAMPLE_BFLOAT16}
CASE_IDS = ["same_format", "mixed_format", "channel_mix_mono", "channel_mix_stereo"]
CANARY = {"int16": 0x5A5A, "float32": 0xC0E00000, "float16": 0xC700, "bfloat16": 0xC0E0, "int64": 0x5A5A5A5A5A5A5A5A}  # -7.0
NAN = {"float32": 0x7FC01234, "float16": 0x7E12, "bfloat16": 0x7FC1}
MINUS_ZERO = {"float32": 0x80000000, "float16": 0x8000, "bfloat16": 0x8000}
_CACHE = {}


class Setup:
    """one case at one T: plan, resampler, windows, the decoded source batch and the oracle's acc, shared by the tests"""

    def __init__(self, engine, corpora, case, frames):
        import torch
        name, channels = case
        images, data, table, headers, rows = corpora[name]
        self.channels, self.frames, self.lengths = channels, frames, [int(v) for v in table["num_samples"]]
        self.d_img = torch.from_numpy(data).cuda()
        if name == "same":
            self.plan = engine.window_decode_plan(headers[0], table)
        elif name == "mixed":
            self.plan = engine.mixed_window_decode_plan(headers, table)
        else:
            self.plan = engine.channel_mix_window_decode_plan(headers, table, channels)
        V = len(RATIOS)
        select = [[v for v in range(V)] for _ in LENGTHS]
        select[0][3] = select[2][0] = None
        self.res = engine.resampler(RATIOS, select)
        self.banks = _banks(self.res)
        self.select = [[ro.NO_BANK if v is None else v for v in row] for row in select]
        self.windows, self.variant = _windows(self.banks, self.select)
        self.n = len(self.windows)
        key = (name, channels, frames)
        if key not in _CACHE:
            _CACHE[key] = ro.expected_acc(rows[channels], self.windows, self.variant, self.select, self.banks, frames, channels)
        self.acc = _CACHE[key]
        self.d_windows = torch.from_numpy(self.windows).cuda()
        self.d_variant = torch.from_numpy(self.variant).cuda()
        self.source = self.res.decode_source(self.plan, self.d_img, self.d_windows, frames, variant=self.d_variant, stats=True)

    def close(self):
        self.res.close()
        self.plan.close()


@pytest.fixture(params=[(c, f) for c in range(len(CASES)) for f in FRAMES], ids=["%s-%d" % (CASE_IDS[c], f) for c in range(len(CASES)) for f in FRAMES])
def setup(request, engine, corpora):  # noqa: F811
    s = Setup(engine, corpora, CASES[request.param[0]], request.param[1])
    yield s
    s.close()


def _view(torch, bits, name):
    """numpy bit patterns -> a cuda tensor of the type"""
    if name == "int64":
        return torch.from_numpy(bits.view(np.int64).copy()).cuda()
    if name == "float32":
        return torch.from_numpy(bits.view(np.int32).copy()).cuda().view(torch.float32)
    return torch.from_numpy(bits.view(np.int16).copy()).cuda().view(getattr(torch, name))


def _host(torch, t, name):
    if name == "int64":
        return t.cpu().numpy().view(np.uint64)
    wide = name == "float32"
    return t.view(torch.int32 if wide else torch.int16).cpu().numpy().view(np.uint32 if wide else np.uint16)


class Bordered:
    """a device buffer of `shape` elements with 16 canary elements on both sides; content: the bit patterns it holds before the run"""

    def __init__(self, torch, shape, name, content):
        self.torch, self.shape, self.name = torch, tuple(shape), name
        self.count = int(np.prod(shape))
        dtype = {"float32": np.uint32, "int64": np.uint64}.get(name, np.uint16)
        bits = np.full(self.count + 32, CANARY[name], dtype=dtype)
        bits[16:16 + self.count] = np.broadcast_to(np.asarray(content, dtype=dtype), self.shape).reshape(-1)
        self.big = _view(torch, bits, name)
        self.view = self.big[16:16 + self.count].view(*self.shape)

    def bits(self):
        host = _host(self.torch, self.big, self.name)
        border = np.concatenate([host[:16], host[16 + self.count:]])
        assert (border == CANARY[self.name]).all(), "wrote outside its buffer"
        got = host[16:16 + self.count].reshape(self.shape)
        return got.view(np.int16) if self.name == "int16" else got


def _random_old(rng, shape, name):
    """random finite values of the type as bit patterns, -0 and +0 among them"""
    import torch
    values = (rng.uniform(-2.0, 2.0, size=shape) * rng.choice([1.0, 2.0 ** -10, 64.0], size=shape)).astype(np.float32)
    bits = np.array(go.bits_of(torch.from_numpy(values).to(go.torch_dtype(name))))
    flat = bits.reshape(-1)
    flat[::7] = MINUS_ZERO[name]
    flat[3::11] = 0
    return bits


def _gains_with_witnesses(s, seed):
    """float32 [N] gains - 1, -1, 0, 1e-41, random ones - and on eight loud windows crafted ones; -> (gains, {type: planted old
    values [(w, c, t, value)]})"""
    rng = np.random.default_rng(seed)
    gains = rng.uniform(-2.0, 2.0, size=s.n).astype(np.float32)
    # the windows with the most elements that float32 does not hold: "exact" needs |acc| > 2^24 and low bits
    inexact = (s.acc.astype(np.float32).astype(np.int64) != s.acc).sum(axis=(1, 2))
    loud = np.argsort(-inexact, kind="stable")[:8].tolist()
    assert inexact[loud[7]] > 16
    quiet = [w for w in range(s.n) if w not in loud[:8] and s.acc[w].any()]
    for w, g in zip(quiet, (1.0, -1.0, 0.0, 1e-41)):
        gains[w] = g
    no_bank = [w for w in range(s.n) if not s.acc[w].any()]
    gains[no_bank[0]], gains[no_bank[1]] = -1.5, 1e-41  # -0 rows, and +0 ones
    planted = {name: [] for name in go.DTYPES}
    jobs = [(kind, name) for name in go.DTYPES for kind in mo.KINDS if (kind, name) != ("double", "float32")]
    for w, (kind, name) in zip(loud, jobs):
        flat = s.acc[w].reshape(-1)
        i, g, old = mo.craft(kind, name, flat, seed)
        gains[w] = g
        if old is not None:
            planted[name].append((w, i // s.frames, i % s.frames, old))
    return gains, planted


def _direct(engine, fn, *args):  # noqa: F811
    cur = engine._enter()
    rc = fn(*args)
    engine._exit(cur)
    engine.synchronize()
    return rc


# ---- gain --------------------------------------------------------------------------------------------------------------------------
def test_rows_with_gain_store_and_add(engine, setup):  # noqa: F811
    import torch
    s = setup
    shape = (s.n, s.channels, s.frames)
    gains, planted = _gains_with_witnesses(s, 31)
    d_gain = torch.from_numpy(gains).cuda()
    rng = np.random.default_rng(77)
    for name in go.DTYPES:
        old = _random_old(rng, shape, name)
        for w, c, t, value in planted[name]:
            old[w, c, t] = go.bits_of(torch.tensor([value], dtype=torch.float32).to(go.torch_dtype(name)))[0]
        # a condition on the inputs: every wrong implementation is caught by some compared element
        found = dict(mo.witnesses(s.acc, gains, name), **mo.witnesses(s.acc, gains, name, old))
        for kind in mo.KINDS:
            if (kind, name) != ("double", "float32"):
                assert found[kind].any(), (kind, name)
        store = Bordered(torch, shape, name, CANARY[name])
        got = s.res.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=store.view, gain=d_gain)
        assert got.data_ptr() == store.view.data_ptr()
        want = mo.expected_rows(s.acc, None, gains, name)
        assert (want == MINUS_ZERO[name]).any()  # a negative gain on zeros
        _compare(store.bits(), want, ("STORE", name), s.windows, s.variant)
        add = Bordered(torch, shape, name, old)
        s.res.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=add.view, gain=d_gain, accumulate=True)
        _compare(add.bits(), mo.expected_rows(s.acc, None, gains, name, old), ("ADD", name), s.windows, s.variant)


# ---- spans -------------------------------------------------------------------------------------------------------------------------
def _spans(n, frames):
    T = frames
    kinds = [(T, 0), (0, 0), (5, 0), (T, 1), (10, T - 1), (10, T), (10, 1 << 40), (-1, 3), (40, 7), (40, 8), (T - 9, 9)]
    if T == 1025:
        kinds.append((600, 700))
    return np.array([kinds[w % len(kinds)] for w in range(n)], dtype=np.int64)


def test_rows_with_spans(engine, setup):  # noqa: F811
    import torch
    s = setup
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
        # STORE into NaNs: every element is defined afterwards
        store = Bordered(torch, shape, name, NAN[name])
        s.res.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=store.view, gain=d_gain, spans=d_spans)
        want = mo.expected_rows(s.acc, spans, gains, name)
        assert not (want == NAN[name]).any() and not (want[~inside] != 0).any()
        _compare(store.bits(), want, ("STORE", name), s.windows, s.variant)
        # ADD: NaNs and -0 outside the spans keep their bits
        old = _random_old(rng, shape, name)
        outside = np.where(rng.integers(0, 2, size=shape) == 1, NAN[name], MINUS_ZERO[name]).astype(old.dtype)
        old[~inside] = outside[~inside]
        add = Bordered(torch, shape, name, old)
        s.res.run_source(s.source, s.frames, s.channels, go.torch_dtype(name), out=add.view, gain=d_gain, accumulate=True, spans=d_spans)
        want = mo.expected_rows(s.acc, spans, gains, name, old)
        assert (want[~inside] == old[~inside]).all()
        _compare(add.bits(), want, ("ADD", name), s.windows, s.variant)
    # spans without a gain table: every gain is 1
    store = Bordered(torch, shape, "float32", NAN["float32"])
    s.res.run_source(s.source, s.frames, s.channels, torch.float32, out=store.view, spans=d_spans)
    _compare(store.bits(), mo.expected_rows(s.acc, spans, None, "float32"), ("STORE", "no gains"), s.windows, s.variant)


# ---- equivalence with the plain run ----------------------------------------------------------------------------------------------------
def test_null_spans_null_gain_store_is_the_plain_run(engine, setup):  # noqa: F811
    import torch
    s = setup
    shape = (s.n, s.channels, s.frames)
    src = s.source
    for name in go.DTYPES:
        plain = s.res.run(s.plan, s.d_img, s.d_windows, s.frames, variant=s.d_variant, dtype=go.torch_dtype(name))
        out = Bordered(torch, shape, name, NAN[name])
        rc = _direct(engine, engine.lib.AADHip_ResamplerRunGain, s.res.handle, s.n, s.channels, src.rows.data_ptr(), src.source_frames,
                     src.lanes.data_ptr(), None, s.frames, KINDS[name], out.view.data_ptr(), None, WINDOW_GAIN_STORE)
        assert rc == AADApiResult.OK
        assert out.bits().tobytes() == _host(torch, plain, name).tobytes(), name
        assert np.array_equal(out.bits(), ro.convert(s.acc, name))


# ---- statistics --------------------------------------------------------------------------------------------------------------------
def test_statistics(engine, setup):  # noqa: F811
    import torch
    s = setup
    shape = (s.n, s.channels, s.frames)
    counts = mo.expected_counts(s.lengths, s.windows, s.variant, s.select, s.banks, s.frames, None)
    # windows inside their stream, across its end, at and behind it, strays
    assert (counts == s.frames).any() and ((counts > 0) & (counts < s.frames)).any() and (counts == 0).any()
    want = mo.expected_stats(s.acc, None, counts)
    no_bank = [w for w in range(s.n) if not s.acc[w].any()]
    assert not want[no_bank].any() and want[..., 2].max() > 1000
    table = Bordered(torch, (s.n, s.channels, 4), "int64", CANARY["int64"])  # pre-filled: every record is overwritten
    got = s.res.run_source(s.source, s.frames, s.channels, stats=table.view, rows=False)
    assert got.data_ptr() == table.view.data_ptr()
    first = table.bits().view(np.int64)
    assert np.array_equal(first, want), np.argwhere(first != want)[:4].tolist()
    again = s.res.run_source(s.source, s.frames, s.channels, stats=True, rows=False)
    assert np.array_equal(again.cpu().numpy(), first)
    # with rows: the four sample types, the rows those of the plain run, the records the same
    for name in DTYPES:
        rows = Bordered(torch, shape, name, CANARY[name])
        table = Bordered(torch, (s.n, s.channels, 4), "int64", 0x33)
        s.res.run_source(s.source, s.frames, s.channels, getattr(torch, name), out=rows.view, stats=table.view)
        _compare(rows.bits(), ro.convert(s.acc, name), ("rows", name), s.windows, s.variant)
        assert np.array_equal(table.bits().view(np.int64), want), name
    # over spans
    spans = _spans(s.n, s.frames)
    counts = mo.expected_counts(s.lengths, s.windows, s.variant, s.select, s.banks, s.frames, spans)
    want = mo.expected_stats(s.acc, spans, counts)
    table = Bordered(torch, (s.n, s.channels, 4), "int64", CANARY["int64"])
    s.res.run_source(s.source, s.frames, s.channels, stats=table.view, rows=False, spans=torch.from_numpy(spans).cuda())
    got = table.bits().view(np.int64)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    # the composed call
    rows, stats = s.res.run(s.plan, s.d_img, s.d_windows, s.frames, variant=s.d_variant, dtype=torch.int16, stats=True)
    assert np.array_equal(stats.cpu().numpy(), first) and np.array_equal(rows.cpu().numpy(), ro.convert(s.acc, "int16"))


# ---- the C calls on hand-made rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", FRAMES)
def test_rails_and_clamps_through_the_c_calls(engine, frames):  # noqa: F811
    import torch
    ratios = [(3, 1), (1, 3), (147, 160)]
    res = engine.resampler(ratios, [[0, 1, 2]])
    try:
        banks = _banks(res)
        t_src = res.source_frames(frames)
        rail = np.full(t_src, -32768, dtype=np.int16)
        square = np.tile(np.repeat(np.array([32767, -32767], dtype=np.int16), 6), t_src // 12 + 1)[:t_src]
        rows, lanes, c_src, acc, counts = [], [], [], [], []
        for b, (L, M, h) in enumerate(banks):
            K = h.shape[1]
            for x, shift, c in ((rail, K // 2 - 1, t_src), (square, K // 2 - 1, t_src), (rail, 0, t_src // 2), (square, 3, 5), (rail, 7, 7)):
                rows.append(x)
                lanes.append((b, shift))
                c_src.append(c)
                acc.append(ro.fir(x, shift, frames, L, M, h))  # the source row as a stream of t_src frames, zeros around it
                counts.append(mo.output_count(c, t_src, shift, L, M, frames))
                assert counts[-1] == mo.output_count_brute(c, t_src, shift, L, M, frames)
        n = len(rows)
        acc = np.array(acc)[:, None, :]
        want = mo.expected_stats(acc, None, np.array(counts))
        assert want[0, 0, 2] == 32768 and want[1, 0, 2] == 32768 and acc[1].max() > 32767 * 16384 + 8192  # the rail; a clamp
        inner = ro.convert(acc[0, 0], "int16") == -32768
        assert inner.sum() > frames // 2 and want[0, 0, 0] >= int(inner.sum()) << 30
        d_rows = torch.from_numpy(np.array(rows)[:, None, :].copy()).cuda()
        d_lanes = torch.from_numpy(np.array(lanes, dtype=np.int32)).cuda()
        source_stats = np.full((n, 1, 4), 0x77, dtype=np.int64)  # the count alone is read
        source_stats[:, 0, 3] = c_src
        d_source_stats = torch.from_numpy(source_stats).cuda()
        lib = engine.lib
        table = Bordered(torch, (n, 1, 4), "int64", CANARY["int64"])
        rc = _direct(engine, lib.AADHip_ResamplerRunStats, res.handle, n, 1, d_rows.data_ptr(), t_src, d_lanes.data_ptr(),
                     d_source_stats.data_ptr(), None, frames, SAMPLE_INT16, None, table.view.data_ptr())
        assert rc == AADApiResult.OK
        got = table.bits().view(np.int64)
        assert np.array_equal(got, want), (got.tolist(), want.tolist())
        out = Bordered(torch, (n, 1, frames), "int16", CANARY["int16"])
        table = Bordered(torch, (n, 1, 4), "int64", 0)
        rc = _direct(engine, lib.AADHip_ResamplerRunStats, res.handle, n, 1, d_rows.data_ptr(), t_src, d_lanes.data_ptr(),
                     d_source_stats.data_ptr(), None, frames, SAMPLE_INT16, out.view.data_ptr(), table.view.data_ptr())
        assert rc == AADApiResult.OK and np.array_equal(table.bits().view(np.int64), want)
        v = out.bits()
        assert np.array_equal(v, ro.convert(acc, "int16")) and v.max() == 32767 and v.min() == -32768
        gains = np.linspace(-1.5, 1.5, n).astype(np.float32)
        d_gain = torch.from_numpy(gains).cuda()
        for name in go.DTYPES:
            out = Bordered(torch, (n, 1, frames), name, NAN[name])
            rc = _direct(engine, lib.AADHip_ResamplerRunGain, res.handle, n, 1, d_rows.data_ptr(), t_src, d_lanes.data_ptr(), None, frames,
                         KINDS[name], out.view.data_ptr(), d_gain.data_ptr(), WINDOW_GAIN_STORE)
            assert rc == AADApiResult.OK
            assert np.array_equal(out.bits(), mo.expected_rows(acc, None, gains, name)), name
        assert np.abs(mo.float_rows(acc)).max() > 1.0
    finally:
        res.close()


# ---- engine level ------------------------------------------------------------------------------------------------------------------
def _oracle_side(engine, decoded, rates, windows, variant, speeds, frames, spans):  # noqa: F811
    """-> (acc [N, 2, T], stats [N, 2, 4]) of one side of the mix, with the library's banks in the order the engine builds them"""
    ratios, select = [], []
    for rate in rates:
        row = []
        for a, b in speeds:
            r = ro.reduce_ratio(16000 * b, rate * a)
            if r not in ratios:
                ratios.append(r)
            row.append(ratios.index(r))
        select.append(row)
    res = engine.resampler(ratios, select)
    try:
        banks = _banks(res)
    finally:
        res.close()
    acc = ro.expected_acc(decoded, windows, variant, select, banks, frames, 2)
    counts = mo.expected_counts([len(d) for d in decoded], windows, variant, select, banks, frames, spans)
    return acc, mo.expected_stats(acc, spans, counts)


def test_mix_windows_resampled(engine):  # noqa: F811
    import torch
    frames = 300
    s_rates, n_rates = [16000, 48000], [48000, 16000, 48000]
    s_images = _encode([3000, 3000], 2, [4, 3], rates=s_rates, seed=5100)
    n_images = _encode([3000, 1500, 400], 2, [3, 4, 2], rates=n_rates, seed=6100)
    s_decoded, n_decoded = [ob.decode(i)[0] for i in s_images], [ob.decode(i)[0] for i in n_images]
    s_data, n_data = torch.from_numpy(_rows(s_images)[0]).cuda(), torch.from_numpy(_rows(n_images)[0]).cuda()
    s_sizes, n_sizes = [len(i) for i in s_images], [len(i) for i in n_images]
    s_windows = np.array([(s, f) for s in range(2) for f in (0, 7, 900, 2800)] + [(2, 0), (1, 2999)], dtype=np.int64)
    n = len(s_windows)
    n_windows = np.array([(k % 3, 37 * k) for k in range(n)], dtype=np.int64)
    n_windows[4] = (3, 0)  # no noise there: gain 0
    spans = np.array([[(120, 40), (300, 0), (7, 293), (50, 299), (0, 0), (300, 1)][k % 6] for k in range(n)], dtype=np.int64)
    for speeds in (((1, 1),), ((1, 1), (11, 10))):
        s_variant = None if len(speeds) == 1 else np.arange(n, dtype=np.int64) % 2
        n_variant = None if len(speeds) == 1 else (np.arange(n, dtype=np.int64) // 2) % 2
        for noise_spans in (None, spans):
            s_acc, s_stats = _oracle_side(engine, s_decoded, s_rates, s_windows, s_variant, speeds, frames, None)
            n_acc, n_stats = _oracle_side(engine, n_decoded, n_rates, n_windows, n_variant, speeds, frames, noise_spans)
            want_gains = snr_gains(torch.from_numpy(s_stats), torch.from_numpy(n_stats), 6.0)
            assert (want_gains > 0).sum() >= n - 4 and want_gains[4] == 0 and want_gains[8] == 0
            for name in ("float32", "bfloat16"):
                rows, gains = engine.mix_windows_resampled(
                    (s_data, s_sizes, torch.from_numpy(s_windows).cuda()), (n_data, n_sizes, torch.from_numpy(n_windows).cuda()), frames, 6.0,
                    16000, speeds=speeds, signal_variant=None if s_variant is None else torch.from_numpy(s_variant).cuda(),
                    noise_variant=None if n_variant is None else torch.from_numpy(n_variant).cuda(), dtype=go.torch_dtype(name),
                    noise_spans=None if noise_spans is None else torch.from_numpy(noise_spans).cuda())
                assert rows.dtype == go.torch_dtype(name) and rows.shape == (n, 2, frames)
                assert torch.equal(gains.cpu(), want_gains), (speeds, noise_spans is not None, name)
                first = mo.expected_rows(s_acc, None, np.ones(n, dtype=np.float32), name)
                want = mo.expected_rows(n_acc, noise_spans, gains.cpu().numpy(), name, first)  # with the RETURNED gains
                assert (want != first).any()
                _compare(_host(torch, rows, name), want, ("mix", speeds, noise_spans is not None, name), s_windows, s_variant)
    levels = engine.window_levels_resampled(n_data, n_sizes, torch.from_numpy(n_windows).cuda(), frames, 16000, speeds=speeds,
                                            variant=torch.from_numpy(n_variant).cuda(), spans=torch.from_numpy(spans).cuda())
    assert np.array_equal(levels.cpu().numpy(), n_stats)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine):  # noqa: F811
    import torch
    lib, bad, ok = engine.lib, AADApiResult.INVALID_ARGUMENT, AADApiResult.OK
    res = engine.resampler([(1, 1), (3, 2)], [[0, 1]])
    try:
        n, ch, frames = 4, 2, 50
        t_src = res.source_frames(frames)
        src = torch.zeros((n, ch, t_src), dtype=torch.int16, device="cuda")
        lanes = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        out = Bordered(torch, (n, ch, frames), "float32", CANARY["float32"])
        stats = Bordered(torch, (n, ch, 4), "int64", CANARY["int64"])
        src_stats = torch.zeros((n, ch, 4), dtype=torch.int64, device="cuda")
        spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        gain = torch.ones(n + 1, dtype=torch.float32, device="cuda")
        sp, ln, op, tp, ss, spn, gp = (t.data_ptr() for t in (src, lanes, out.view, stats.view, src_stats, spans, gain))
        f32, h = SAMPLE_FLOAT32, res.handle

        def run_gain(**k):
            a = dict(h=h, n=n, ch=ch, sp=sp, t_src=t_src, ln=ln, spans=spn, frames=frames, kind=f32, op=op, gain=gp, mode=WINDOW_GAIN_STORE)
            a.update(k)
            return lib.AADHip_ResamplerRunGain(a["h"], a["n"], a["ch"], a["sp"], a["t_src"], a["ln"], a["spans"], a["frames"], a["kind"],
                                               a["op"], a["gain"], a["mode"])

        def run_stats(**k):
            a = dict(h=h, n=n, ch=ch, sp=sp, t_src=t_src, ln=ln, ss=ss, spans=None, frames=frames, kind=f32, op=op, tp=tp)
            a.update(k)
            return lib.AADHip_ResamplerRunStats(a["h"], a["n"], a["ch"], a["sp"], a["t_src"], a["ln"], a["ss"], a["spans"], a["frames"],
                                                a["kind"], a["op"], a["tp"])

        # AADHip_ResamplerRun's errors, kept by both
        for k in (dict(h=None), dict(sp=None), dict(ln=None), dict(ch=0), dict(frames=0), dict(t_src=t_src - 1), dict(kind=2), dict(kind=-1),
                  dict(sp=sp + 1), dict(ln=ln + 2), dict(op=op + 2), dict(n=1 << 62)):
            assert run_gain(**k) == bad, k
            assert run_stats(**k) == bad, k
        assert run_gain(op=None) == bad
        # their own
        assert run_gain(kind=SAMPLE_INT16) == bad
        for mode in (2, -1):
            assert run_gain(mode=mode) == bad
        assert run_gain(gain=gp + 2) == bad and run_gain(spans=spn + 4) == bad
        assert run_stats(spans=spn + 4, op=None) == bad
        assert run_stats(tp=tp + 4) == bad and run_stats(ss=ss + 4) == bad
        assert run_stats(tp=None) == bad and run_stats(ss=None) == bad
        assert run_stats(spans=spn) == bad  # rows together with spans
        assert run_stats(kind=3, op=None) == bad  # the sample type is validated without rows too
        # N * C * 32 bytes past 64 bits where N * C * T * 4 and N * C * T_src * 2 are not: T = 1
        identity = engine.resampler([(1, 1)], [[0]])
        try:
            t1 = identity.source_frames(1)
            many = (1 << 59) + 5
            assert many * 32 >= 1 << 64 > many * t1 * 2 and many * 4 < 1 << 64
            assert run_stats(h=identity.handle, n=many, ch=1, frames=1, t_src=t1, op=None) == bad
            assert run_stats(h=identity.handle, n=many - 10, ch=1, frames=1, t_src=t1, op=None, tp=None) == bad  # null table, sizes fine
        finally:
            identity.close()
        assert "resampler" in engine.last_error()
        assert run_gain(n=0) == ok and run_stats(n=0) == ok and run_stats(n=0, tp=None, ss=None) == ok  # no window: no launch
        engine.synchronize()
        out.bits()
        stats.bits()
        assert (_host(torch, out.view, "float32") == CANARY["float32"]).all()
        assert (_host(torch, stats.view, "int64") == CANARY["int64"]).all()
        # and the good calls are good
        assert _direct(engine, run_gain) == ok and _direct(engine, lambda: run_stats(op=None)) == ok
        assert not (_host(torch, out.view, "float32") == CANARY["float32"]).any()
        assert not stats.bits().any()
    finally:
        res.close()
