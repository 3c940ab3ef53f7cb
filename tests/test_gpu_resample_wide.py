"""The wide resampler on the device (AADHip_ResamplerCreateWide; aad_amd/csrc/aad_resample_wide.hip): ratios whose bank does not
fit a workgroup's LDS, the bank rows gathered per round of outputs.

Bar: bit for bit against tests/resample_oracle.py and tests/resample_mix_oracle.py with the library's own banks (which
tests/test_resample_wide_host.py holds to the oracle's construction), canaries on both sides of every buffer, at T = 257 and
T = 1025 - one output past a gather round of 256 and one past the tile of 1024 -
  * a corpus of its own, made by the planar encoder (Engine.encode_planar): streams of 700, 14000, 14000 and 40 frames, so that
    for every ratio a window has all taps of its last output inside its stream (1025/10933 at T = 1025 reads 11178 source
    frames; asserted on the CPU), in the three kinds of window decode plan: same format, mixed formats, mono + stereo into two
    channels;
  * in ONE wide resampler 1600/3969, 1600/4851, 1600/1617 (the 44.1 kHz corpus), 1025/1, 1024/1367 (L within the old limit, the
    bank above 64 KB), 1025/10933 (K = 256) and 4099/4098 with the resident 1/1, 10/9 and 160/441; its round is that of K = 256,
    64 outputs.  Two more resamplers bring the other rounds: 1600/3969, 1600/4851 and 4099/4098 with 1/1 (256 outputs) and
    331/1370, K = 100, with 1600/3969 and 10/9 (128 outputs);
  * windows at frame 0, below, at and above each bank's lead, inside the stream, across its end, at and behind it, stray streams
    and variants, wrapped and huge values, a select entry of 0xFFFF;
  * the plain run into the four sample types; gain x the three float types x STORE / ADD with crafted gains, spans (clipped,
    empty, odd offsets, across element 1024; STORE into NaNs, ADD over NaNs and -0) and statistics with and without rows and
    spans, `count` against the brute force over num_samples: the tests of tests/test_gpu_resample_mix.py, run over these setups;
  * WITNESSES, asserted on the CPU before the device is asked: for every gathered ratio some compared output changes bits when
    its taps come from the neighbouring output's phase, from the phase of the output 256 further on, or from phase p of a
    resident-sized prefix of the bank (p mod the phases that fit 64 KB; 1025/1 reaches phase 1024 at T = 1025 alone) - a wrong
    row cannot pass;
  * the resident banks through the wide resampler byte for byte those of a plain resampler: four types, gain, statistics;
  * Engine.decode_windows_resampled(..., 16000, speeds=((9, 10), (1, 1), (11, 10)), wide=True) over 16 / 44.1 / 48 kHz headers
    for all nine (stream, speed) pairs, refused without `wide`; window_levels_resampled and mix_windows_resampled with wide=True,
    the returned gains included;
  * the wide constructor's refusals and the runs' on a wide resampler, which leave canaries untouched."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import resample_mix_oracle as mo
import resample_oracle as ro
import test_gpu_resample_mix as mix
import window_gain_oracle as go
from aad_amd.capi import (AADApiResult, AADHipResampleRatio, ApiError, SAMPLE_FLOAT32, STREAM_DESC_DTYPE, WINDOW_GAIN_STORE,
                          make_parameter)
from aad_amd.engine import parse_header, snr_gains
from aad_amd.synth import synth_pcm
from channel_mix_oracle import mix_stream
from test_gpu_window_resample import DTYPES, FRAMES, _banks, _compare, _run, engine  # noqa: F401

pytestmark = pytest.mark.gpu

LENGTHS = [700, 14000, 14000, 40]
RESIDENT = [(1, 1), (10, 9), (160, 441)]
# name -> ratios, one wide resampler each; the round follows from the gathered bank with the most taps (aad_resample.h)
SETS = {"all": [(1600, 3969), (1600, 4851), (1600, 1617), (1025, 1), (1024, 1367), (1025, 10933), (4099, 4098)] + RESIDENT,
        "round256": [(1600, 3969), (1600, 4851), (4099, 4098), (1, 1)],
        "round128": [(331, 1370), (1600, 3969), (10, 9)]}
TAPS = {(1600, 3969): 60, (1600, 4851): 74, (1600, 1617): 26, (1025, 1): 24, (1024, 1367): 34, (1025, 10933): 256, (4099, 4098): 24,
        (1, 1): 2, (10, 9): 24, (160, 441): 68, (331, 1370): 100}
CASES = {"same_format": ("same", 2), "mixed_format": ("mixed", 1), "channel_mix_stereo": ("mix", 2)}
SETUPS = [("all", c, f) for c in CASES for f in FRAMES] + [(s, "same_format", f) for s in ("round256", "round128") for f in FRAMES]
_ACC = {}


def _gathered(L, M):
    return not ro.limits_ok(L, M)


# ---- the corpus --------------------------------------------------------------------------------------------------------------------
def _encode_planar(engine, torch, lengths, channels, bits, rates=None, seed=7300):  # noqa: F811
    """one image per stream from the planar encoder -> (uint8 [S, pitch], STREAM_DESC_DTYPE table, sizes, headers, decoded rows)"""
    images = []
    for i, n in enumerate(lengths):
        ch = channels[i] if isinstance(channels, (list, tuple)) else channels
        b = bits[i] if isinstance(bits, (list, tuple)) else bits
        pcm = synth_pcm(1, n, ch, seed=seed + 17 * i)[0]  # [n, ch]
        x = torch.from_numpy(np.ascontiguousarray(pcm.T[None])).cuda()
        d_img, sizes = engine.encode_planar(x, make_parameter(ch, b, 256, rates[i] if rates else 48000, False, 0))
        images.append(bytes(d_img[0, :sizes[0]].cpu().numpy()))
    pitch = -(-max(len(i) for i in images) // 64) * 64 + 64
    data = np.zeros((len(images), pitch), dtype=np.uint8)
    table = np.zeros(len(images), dtype=STREAM_DESC_DTYPE)
    for i, img in enumerate(images):
        data[i, :len(img)] = np.frombuffer(img, dtype=np.uint8)
        table["data_offset"][i], table["data_size"][i] = i * pitch, len(img)
        table["num_samples"][i] = parse_header(img[:31]).num_samples
    headers = [parse_header(img[:31]) for img in images]
    decoded = [ob.decode(img)[0] for img in images]
    assert [len(d) for d in decoded] == list(lengths)
    return data, table, [len(i) for i in images], headers, decoded


@pytest.fixture(scope="module")
def corpora(engine):  # noqa: F811
    """name -> (data [S, pitch], table, headers, {channels: int16 rows per stream the plan of that kind decodes})"""
    import torch
    out = {}
    for name, channels, bits in (("same", 2, 4), ("mixed", 1, [4, 3, 2, 4]), ("mix", [1, 2, 2, 1], [4, 3, 4, 2])):
        data, table, _, headers, decoded = _encode_planar(engine, torch, LENGTHS, channels, bits)
        rows = {2: [mix_stream(d, 2) for d in decoded]} if name == "mix" else {channels: decoded}
        out[name] = (data, table, headers, rows)
    return out


def _windows(banks, select):
    """windows and variants: per variant (bank) the edges of its own K on a stream of 14000 frames, then the strays"""
    rows, variant = [], []
    for v, (L, M, h) in enumerate(banks):
        K = h.shape[1]
        s = 1 + v % 2
        n = LENGTHS[s]
        firsts = [0, 1, max(K // 2 - 2, 0), K // 2 - 1, K // 2, 1234, n - 100, n - 1, n, n + K // 2 - 2, n + K]
        rows += [(s, f) for f in firsts] + [(0, 0), (0, 650), (3, 0), (3, 39), (3, 40)]
        variant += [v] * (len(firsts) + 5)
    V = len(banks)
    strays = [((len(LENGTHS), 5), 0), ((-1, 5), 0), (((1 << 63) - 1, 0), 1),      # no such stream
              ((1, 5), V), ((1, 5), -1), ((1, 5), 1 << 40),                     # no such variant
              ((1, -1), 1), ((2, 1 << 40), 2), ((2, -(1 << 62)), 0), ((1, (1 << 63) - 1), 1)]  # wrapped and huge starts
    rows += [s[0] for s in strays]
    variant += [s[1] for s in strays]
    none = [(s, v) for s in range(len(select)) for v in range(V) if select[s][v] == ro.NO_BANK]
    rows += [(s, 7) for s, v in none]
    variant += [v for s, v in none]
    return np.array(rows, dtype=np.int64), np.array(variant, dtype=np.int64)


# ---- witnesses ---------------------------------------------------------------------------------------------------------------------
def _fir_with_phases(x, first, frames, L, M, h, p):
    """ro.fir with the taps of output n taken from phase p[n]; the window lies inside the stream"""
    K = h.shape[1]
    n = np.arange(frames, dtype=np.int64)
    at = first + (n * M // L)[:, None] + np.arange(K)[None, :] - (K // 2 - 1)
    assert at.min() >= 0 and at.max() < len(x)
    return (h[p].astype(np.int64) * np.asarray(x, dtype=np.int64)[at]).sum(axis=1)


def _assert_witnesses(s):
    """for every gathered bank of the setup: a compared window inside its stream on which each wrong row changes bits"""
    for v, (L, M, h) in enumerate(s.banks):
        if not _gathered(L, M):
            continue
        K = h.shape[1]
        reach = (s.frames - 1) * M // L + K - (K // 2 - 1)  # frames from a window's first to its last output's last tap
        inside = [w for w, (stream, first) in enumerate(s.windows.tolist())  # Python integers: the strays are huge
                  if s.variant[w] == v and 0 <= stream < len(LENGTHS) and s.select[stream][v] == v
                  and K // 2 - 1 <= first and first + reach <= LENGTHS[stream]]
        assert inside, ("no window with every tap of its last output inside the stream", L, M, s.frames)
        w = inside[-1]
        stream, first = (int(t) for t in s.windows[w])
        x = s.rows_of[stream][:, 0]
        n = np.arange(s.frames, dtype=np.int64)
        p = n * M % L
        right = _fir_with_phases(x, first, s.frames, L, M, h, p)
        assert np.array_equal(right, s.acc[w, 0]), (L, M)
        prefix = min(1024, 65536 // (2 * K))  # the phases of a bank that fits LDS whole
        wrong = {"the neighbouring output's phase": (n + 1) * M % L, "the phase of the output 256 further on": (n + 256) * M % L,
                 "phase p of a resident-sized prefix": p % prefix}
        if s.frames < L and (p < prefix).all():  # 1025/1 at T = 257 uses phases 0 ... 256 alone; at T = 1025 it reaches 1024
            assert (L, M, s.frames) == (1025, 1, 257)
            del wrong["phase p of a resident-sized prefix"]
        for what, q in wrong.items():
            other = _fir_with_phases(x, first, s.frames, L, M, h, q)
            for name in ("int16", "float32"):
                assert (ro.convert(other, name) != ro.convert(right, name)).any(), (what, L, M, name)


# ---- setups ------------------------------------------------------------------------------------------------------------------------
class Setup:
    """one ratio set, one kind of plan, one T: what tests/test_gpu_resample_mix.py's Setup holds, over a wide resampler"""

    def __init__(self, engine, corpora, ratios_name, case, frames):  # noqa: F811
        import torch
        name, channels = CASES[case]
        data, table, headers, rows = corpora[name]
        ratios = SETS[ratios_name]
        self.channels, self.frames, self.lengths = channels, frames, [int(v) for v in table["num_samples"]]
        self.rows_of = rows[channels]
        self.d_img = torch.from_numpy(data).cuda()
        if name == "same":
            self.plan = engine.window_decode_plan(headers[0], table)
        elif name == "mixed":
            self.plan = engine.mixed_window_decode_plan(headers, table)
        else:
            self.plan = engine.channel_mix_window_decode_plan(headers, table, channels)
        V = len(ratios)
        select = [[v for v in range(V)] for _ in LENGTHS]
        select[0][1] = select[2][0] = None  # 0xFFFF
        self.res = engine.resampler(ratios, select, wide=True)
        self.banks = _banks(self.res)
        assert [(L, M) for L, M, _ in self.banks] == ratios and [h.shape[1] for _, _, h in self.banks] == [TAPS[r] for r in ratios]
        self.select = [[ro.NO_BANK if v is None else v for v in row] for row in select]
        self.windows, self.variant = _windows(self.banks, self.select)
        self.n = len(self.windows)
        assert self.res.source_frames(frames) == ro.source_frames(frames, [(L, M, h.shape[1]) for L, M, h in self.banks])
        key = (ratios_name, case, frames)
        if key not in _ACC:
            _ACC[key] = ro.expected_acc(self.rows_of, self.windows, self.variant, self.select, self.banks, frames, channels)
        self.acc = _ACC[key]
        assert (self.acc != 0).any(axis=(1, 2)).sum() > self.n // 2
        _assert_witnesses(self)
        self.d_windows = torch.from_numpy(self.windows).cuda()
        self.d_variant = torch.from_numpy(self.variant).cuda()
        self.source = self.res.decode_source(self.plan, self.d_img, self.d_windows, frames, variant=self.d_variant, stats=True)

    def close(self):
        self.res.close()
        self.plan.close()


@pytest.fixture(params=SETUPS, ids=["%s-%s-%d" % s for s in SETUPS])
def setup(request, engine, corpora):  # noqa: F811
    s = Setup(engine, corpora, *request.param)
    yield s
    s.close()


def test_the_largest_ratio_reads_11178_source_frames():
    assert ro.source_frames(1025, [(1025, 10933, 256)]) == 11178 and 1234 + 11178 - 127 <= LENGTHS[1]


# ---- rows, gain, spans, statistics against the oracles ---------------------------------------------------------------------------------
def test_rows_equal_the_definition(engine, setup):  # noqa: F811
    import torch
    s = setup
    for dtype in DTYPES:
        got = _run(torch, s.res, s.plan, s.d_img, s.windows, s.variant, s.frames, s.channels, dtype)
        _compare(got, ro.convert(s.acc, dtype), (dtype,), s.windows, s.variant)
    acc0 = ro.expected_acc(s.rows_of, s.windows, None, s.select, s.banks, s.frames, s.channels)  # no variant table: all 0
    _compare(_run(torch, s.res, s.plan, s.d_img, s.windows, None, s.frames, s.channels, "int16"), ro.convert(acc0, "int16"),
             ("no variants",), s.windows, None)


def test_rows_with_gain_store_and_add(engine, setup):  # noqa: F811
    mix.test_rows_with_gain_store_and_add(engine, setup)


def test_rows_with_spans(engine, setup):  # noqa: F811
    if setup.frames == 1025:
        assert (600, 700) in [tuple(v) for v in mix._spans(setup.n, setup.frames).tolist()]  # a span across element 1024
    mix.test_rows_with_spans(engine, setup)


def test_null_spans_null_gain_store_is_the_plain_run(engine, setup):  # noqa: F811
    mix.test_null_spans_null_gain_store_is_the_plain_run(engine, setup)


def test_statistics(engine, setup):  # noqa: F811
    mix.test_statistics(engine, setup)


# ---- resident banks: the plain resampler's bytes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", FRAMES)
def test_resident_banks_equal_a_plain_resampler(engine, corpora, frames):  # noqa: F811
    import torch
    s = Setup(engine, corpora, "all", "same_format", frames)
    plain = None
    try:
        first = SETS["all"].index(RESIDENT[0])
        assert SETS["all"][first:] == RESIDENT
        keep = [w for w in range(s.n) if first <= s.variant[w] < first + len(RESIDENT)]
        windows = np.ascontiguousarray(s.windows[keep])
        variant = np.ascontiguousarray(s.variant[keep]) - first
        select = [[None if v == ro.NO_BANK else v - first for v in row[first:]] for row in s.select]
        plain = engine.resampler(RESIDENT, select)
        assert (s.acc[keep] != 0).any(axis=(1, 2)).sum() > len(keep) // 2
        d_windows = torch.from_numpy(windows).cuda()
        shape = (len(keep), s.channels, frames)
        gains = np.random.default_rng(9).uniform(-2.0, 2.0, size=len(keep)).astype(np.float32)
        d_gain = torch.from_numpy(gains).cuda()
        spans = mix._spans(len(keep), frames)
        d_spans = torch.from_numpy(spans).cuda()
        got = {}
        for label, res, var in (("wide", s.res, variant + first), ("plain", plain, variant)):
            out = got[label] = {}
            d_variant = torch.from_numpy(var).cuda()
            source = res.decode_source(s.plan, s.d_img, d_windows, frames, variant=d_variant, stats=True)
            for name in DTYPES:
                rows = mix.Bordered(torch, shape, name, mix.CANARY[name])
                table = mix.Bordered(torch, shape[:2] + (4,), "int64", mix.CANARY["int64"])
                res.run_source(source, frames, s.channels, getattr(torch, name), out=rows.view)
                out["rows", name] = rows.bits().tobytes()
                res.run_source(source, frames, s.channels, getattr(torch, name), out=rows.view, stats=table.view)
                out["stats rows", name] = rows.bits().tobytes() + table.bits().tobytes()
            for name in go.DTYPES:
                old = mix._random_old(np.random.default_rng(11), shape, name)
                for accumulate in (False, True):
                    rows = mix.Bordered(torch, shape, name, old)
                    res.run_source(source, frames, s.channels, go.torch_dtype(name), out=rows.view, gain=d_gain, accumulate=accumulate,
                                   spans=d_spans)
                    out["gain", name, accumulate] = rows.bits().tobytes()
            for with_spans in (None, d_spans):
                table = mix.Bordered(torch, shape[:2] + (4,), "int64", mix.CANARY["int64"])
                res.run_source(source, frames, s.channels, stats=table.view, rows=False, spans=with_spans)
                out["stats", with_spans is not None] = table.bits().tobytes()
        assert got["wide"].keys() == got["plain"].keys()
        for key in got["wide"]:
            assert got["wide"][key] == got["plain"][key], key
        assert got["wide"]["rows", "int16"] == ro.convert(s.acc[keep], "int16").tobytes()
    finally:
        if plain is not None:
            plain.close()
        s.close()


# ---- engine level ------------------------------------------------------------------------------------------------------------------
SPEEDS = ((9, 10), (1, 1), (11, 10))
RATES = [16000, 44100, 48000]


def _oracle_side(engine, decoded, rates, windows, variant, speeds, frames, spans):  # noqa: F811
    """-> (acc [N, 2, T], stats [N, 2, 4], ratios) of one corpus at 16 kHz, with the library's banks in the order the engine builds them"""
    ratios, select = [], []
    for rate in rates:
        row = []
        for a, b in speeds:
            r = ro.reduce_ratio(16000 * b, rate * a)
            if r not in ratios:
                ratios.append(r)
            row.append(ratios.index(r))
        select.append(row)
    res = engine.resampler(ratios, select, wide=True)
    try:
        banks = _banks(res)
    finally:
        res.close()
    acc = ro.expected_acc(decoded, windows, variant, select, banks, frames, 2)
    counts = mo.expected_counts([len(d) for d in decoded], windows, variant, select, banks, frames, spans)
    return acc, mo.expected_stats(acc, spans, counts), ratios


@pytest.fixture(scope="module")
def rate_corpus(engine):  # noqa: F811
    import torch
    lengths = [3000, 6000, 6000]
    data, _, sizes, headers, decoded = _encode_planar(engine, torch, lengths, 2, [4, 3, 2], rates=RATES, seed=8100)
    assert [h.sampling_rate for h in headers] == RATES
    return torch.from_numpy(data).cuda(), sizes, decoded


def test_decode_windows_resampled_over_the_three_rate_corpus(engine, rate_corpus):  # noqa: F811
    import torch
    d_img, sizes, decoded = rate_corpus
    frames = 700  # two rounds of 256 and most of a third
    pairs = [(s, v) for s in range(3) for v in range(3)]
    windows = np.array([(s, f) for s, v in pairs for f in (0, 40, 900)] + [(3, 0), (1, 5990), (1, -1)], dtype=np.int64)
    variant = np.array([v for s, v in pairs for _ in range(3)] + [0, 0, 2], dtype=np.int64)
    acc, stats, ratios = _oracle_side(engine, decoded, RATES, windows, variant, SPEEDS, frames, None)
    assert (1600, 3969) in ratios and (1600, 4851) in ratios and len(ratios) == 9
    for k, (s, v) in enumerate(pairs):  # all nine (stream, speed) pairs give rows that are not silence
        assert acc[3 * k:3 * k + 3].any(axis=(1, 2)).all(), (s, v)
    d_windows, d_variant = torch.from_numpy(windows).cuda(), torch.from_numpy(variant).cuda()
    for name in ("int16", "float32"):
        got = engine.decode_windows_resampled(d_img, sizes, d_windows, frames, 16000, speeds=SPEEDS, variant=d_variant,
                                              dtype=getattr(torch, name), wide=True)
        _compare(mix._host(torch, got, name).view(np.int16 if name == "int16" else np.uint32), ro.convert(acc, name), (name,), windows, variant)
    rows, table = engine.decode_windows_resampled(d_img, sizes, d_windows, frames, 16000, speeds=SPEEDS, variant=d_variant,
                                                  dtype=torch.bfloat16, return_stats=True, wide=True)
    _compare(mix._host(torch, rows, "bfloat16"), ro.convert(acc, "bfloat16"), ("bfloat16",), windows, variant)
    assert np.array_equal(table.cpu().numpy(), stats)
    # without `wide` the 44.1 kHz stream is refused, as before
    for kwargs in ({}, dict(wide=False)):
        with pytest.raises(ApiError) as refused:
            engine.decode_windows_resampled(d_img, sizes, d_windows, frames, 16000, speeds=SPEEDS, variant=d_variant, **kwargs)
        assert refused.value.code == AADApiResult.INVALID_ARGUMENT


def test_levels_and_mix_over_the_three_rate_corpus(engine, rate_corpus):  # noqa: F811
    import torch
    d_img, sizes, decoded = rate_corpus
    frames = 700
    n = 12
    s_windows = np.array([(k % 3, 31 * k) for k in range(n)], dtype=np.int64)
    n_windows = np.array([((k + 1) % 3, 1000 + 53 * k) for k in range(n)], dtype=np.int64)
    n_windows[4] = (3, 0)  # no noise there: gain 0
    s_variant = np.arange(n, dtype=np.int64) % 3
    n_variant = (np.arange(n, dtype=np.int64) // 3) % 3
    spans = np.array([[(320, 40), (700, 0), (7, 693), (50, 699), (0, 0), (700, 1)][k % 6] for k in range(n)], dtype=np.int64)
    tensors = [torch.from_numpy(a).cuda() for a in (s_windows, n_windows, s_variant, n_variant, spans)]
    d_sw, d_nw, d_sv, d_nv, d_spans = tensors
    s_acc, s_stats, _ = _oracle_side(engine, decoded, RATES, s_windows, s_variant, SPEEDS, frames, None)
    for noise_spans, d_noise_spans in ((None, None), (spans, d_spans)):
        n_acc, n_stats, _ = _oracle_side(engine, decoded, RATES, n_windows, n_variant, SPEEDS, frames, noise_spans)
        levels = engine.window_levels_resampled(d_img, sizes, d_nw, frames, 16000, speeds=SPEEDS, variant=d_nv, spans=d_noise_spans, wide=True)
        assert np.array_equal(levels.cpu().numpy(), n_stats)
        want_gains = snr_gains(torch.from_numpy(s_stats), torch.from_numpy(n_stats), 6.0)
        assert (want_gains > 0).sum() >= n - 3 and want_gains[4] == 0
        for name in ("float32", "float16"):
            rows, gains = engine.mix_windows_resampled((d_img, sizes, d_sw), (d_img, sizes, d_nw), frames, 6.0, 16000, speeds=SPEEDS,
                                                       signal_variant=d_sv, noise_variant=d_nv, dtype=go.torch_dtype(name),
                                                       noise_spans=d_noise_spans, wide=True)
            assert torch.equal(gains.cpu(), want_gains), (noise_spans is not None, name)
            first = mo.expected_rows(s_acc, None, np.ones(n, dtype=np.float32), name)
            want = mo.expected_rows(n_acc, noise_spans, gains.cpu().numpy(), name, first)  # with the RETURNED gains
            assert (want != first).any()
            _compare(mix._host(torch, rows, name), want, ("mix", noise_spans is not None, name), s_windows, s_variant)
    with pytest.raises(ApiError) as refused:
        engine.window_levels_resampled(d_img, sizes, d_nw, frames, 16000, speeds=SPEEDS, variant=d_nv)
    assert refused.value.code == AADApiResult.INVALID_ARGUMENT


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine):  # noqa: F811
    import torch
    lib, R = engine.lib, AADApiResult
    create = lib.AADHip_ResamplerCreateWide
    sel = (C.c_uint16 * 2)(0, 0xFFFF)
    ratio = lambda *pairs: (AADHipResampleRatio * len(pairs))(*[AADHipResampleRatio(u, d) for u, d in pairs])
    for pairs in ([(0, 1)], [(1, 0)], [(32769, 1)], [(1025, 11000)], [(32768, 43691)], [(1, 11)]):
        handle = C.c_void_p(0x55)
        assert create(engine._ctx, 1, ratio(*pairs), 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT, pairs
        assert handle.value is None
        assert "wide resampler" in engine.last_error()
    handle = C.c_void_p(0x55)
    bad_sel = (C.c_uint16 * 2)(0, 1)
    assert create(engine._ctx, 1, ratio((1600, 3969)), 1, 2, bad_sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert create(engine._ctx, 1, ratio((1600, 3969)), 1, 0, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert create(engine._ctx, 0, ratio((1600, 3969)), 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert create(engine._ctx, 0xFFFF, ratio((1600, 3969)), 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert create(engine._ctx, 1, None, 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert create(engine._ctx, 1, ratio((1600, 3969)), 1, 2, None, C.byref(handle)) == R.INVALID_ARGUMENT
    assert create(engine._ctx, 1, ratio((1600, 3969)), 1, 2, sel, None) == R.INVALID_ARGUMENT
    assert create(None, 1, ratio((1600, 3969)), 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    for pairs, shape in (([(32768, 43689)], (32768, 43689, 32)), ([(1025, 10933)], (1025, 10933, 256))):  # the largest bank, the most taps
        assert create(engine._ctx, 1, ratio(*pairs), 1, 2, sel, C.byref(handle)) == R.OK, pairs
        L, M, K = C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert lib.AADHip_ResamplerBank(handle, 0, C.byref(L), C.byref(M), C.byref(K), None, 0) == R.OK
        assert (L.value, M.value, K.value) == shape
        lib.AADHip_ResamplerDestroy(handle)
    # the runs keep their errors on a wide resampler
    res = engine.resampler([(1600, 3969), (1, 1)], [[0, 1]], wide=True)
    try:
        n, ch, frames = 4, 2, 300
        t_src = res.source_frames(frames)
        assert t_src == 299 * 3969 // 1600 + 60
        src = torch.zeros((n, ch, t_src), dtype=torch.int16, device="cuda")
        lanes = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        out = mix.Bordered(torch, (n, ch, frames), "float32", mix.CANARY["float32"])
        stats = mix.Bordered(torch, (n, ch, 4), "int64", mix.CANARY["int64"])
        src_stats = torch.zeros((n, ch, 4), dtype=torch.int64, device="cuda")
        sp, ln, op, tp, ss = (t.data_ptr() for t in (src, lanes, out.view, stats.view, src_stats))
        f32, h, bad = SAMPLE_FLOAT32, res.handle, R.INVALID_ARGUMENT
        count = C.c_uint32(9)
        assert lib.AADHip_ResamplerSourceFrames(h, 0, C.byref(count)) == bad and count.value == 9
        assert lib.AADHip_ResamplerSourceFrames(h, (1 << 31) // 3969 + 2, C.byref(count)) == bad and count.value == 9  # (T - 1) M >= 2^31
        small = np.full(10, 77, dtype=np.int16)
        L, M, K = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
        assert lib.AADHip_ResamplerBank(h, 0, C.byref(L), C.byref(M), C.byref(K), small.ctypes.data, 10) == R.INSUFFICIENT_BUFFER
        assert (L.value, M.value, K.value) == (9, 9, 9) and (small == 77).all()
        run, gain, stat = lib.AADHip_ResamplerRun, lib.AADHip_ResamplerRunGain, lib.AADHip_ResamplerRunStats
        for k in (dict(sp=None), dict(ln=None), dict(ch=0), dict(frames=0), dict(t_src=t_src - 1), dict(kind=2), dict(sp=sp + 1),
                  dict(ln=ln + 2), dict(op=op + 2), dict(n=1 << 62)):
            a = dict(n=n, ch=ch, sp=sp, t_src=t_src, ln=ln, frames=frames, kind=f32, op=op)
            a.update(k)
            assert run(h, a["n"], a["ch"], a["sp"], a["t_src"], a["ln"], a["frames"], a["kind"], a["op"]) == bad, k
            assert gain(h, a["n"], a["ch"], a["sp"], a["t_src"], a["ln"], None, a["frames"], a["kind"], a["op"], None, WINDOW_GAIN_STORE) == bad, k
            assert stat(h, a["n"], a["ch"], a["sp"], a["t_src"], a["ln"], ss, None, a["frames"], a["kind"], a["op"], tp) == bad, k
        assert run(h, n, ch, sp, t_src, ln, frames, f32, None) == bad
        assert gain(h, n, ch, sp, t_src, ln, None, frames, f32, op, None, 2) == bad
        assert stat(h, n, ch, sp, t_src, ln, ss, None, frames, f32, op, None) == bad
        assert "resampler" in engine.last_error()
        assert run(h, 0, ch, sp, t_src, ln, frames, f32, op) == R.OK  # no window: no launch
        engine.synchronize()
        assert (out.bits() == mix.CANARY["float32"]).all()
        assert (stats.bits() == mix.CANARY["int64"]).all()
        # and the good calls are good: lanes {bank 0, shift 0} over a silent source batch give +0 rows and zero records
        assert mix._direct(engine, run, h, n, ch, sp, t_src, ln, frames, f32, op) == R.OK
        assert not out.bits().any()
        assert mix._direct(engine, stat, h, n, ch, sp, t_src, ln, ss, None, frames, f32, None, tp) == R.OK
        assert not stats.bits().any()
    finally:
        res.close()
