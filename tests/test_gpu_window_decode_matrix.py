"""Window decode, every compiled kernel: each record of tests/window_matrix.py's case table names one case of this file, and each
case runs every entry point over its plan - AADHip_WindowDecodePlanRun in int16, float32, float16 and bfloat16; ...RunStats with
rows of the four types and without rows; ...RunGain and ...RunPlaced in the three float types, STORE and ADD; ...RunPlacedStats.

Bar: every row EQUALS, as bit patterns, the oracle's (tests/window_oracle.py, channel_mix_oracle.py, window_half_oracle.py,
window_gain_oracle.py, window_placed_oracle.py), every statistics record the integers of window_stats_oracle.py; rows, records and
the window, span and gain tables lie between 64-byte canaries.  No tolerance anywhere.

Corpora (built once, on the CPU: matrix_case): streams of about 2.5 blocks, 48 <= spb <= 160, ragged lengths, stream CUT truncated
inside its last block.  Same format: the twelve geometries.  Mixed: a mono, a stereo (all six variants) and a 3-channel plan, two
block sizes each.  Channel mix: all nine source variants, into one and into two rows.  One T = (3 max_spb) // 2 | 1 per case; per
stream windows at phase 0, 3 and spb - 1, one ending at the stream's end, one starting on its last frame; a past-the-end window and
two stray ones per case.

Every cell must do work: before a run, every variant of the plan has a window on one of its streams whose expected rows are not
zero.  The gain and placed runs also carry the VECTOR-PATH WITNESSES of one stream per variant (window_gain_oracle.
vector_witnesses): elements behind a block's header samples, which leave through WindowRow::chunk() - sixteen at a time, pairs
packed into one word, the old values of ADD loaded as 16-byte vectors - with a gain (and under ADD an old value) on which a skipped
float32 rounding, a fused multiply-add or a gain applied before the scale gives other bits.  One window per witness, four per
stream and kind: both halves of a packed word x both put8 calls of a chunk.  tests/test_window_gain_host.py confirms each exactly."""
import collections
import functools

import numpy as np
import pytest

import oracle_binding as ob
import window_gain_oracle as go
import window_matrix as wm
import window_placed_oracle as po
from aad_amd.engine import parse_header
from channel_mix_oracle import channel_mix_expected
from test_gpu_window_decode import _pack
from test_gpu_window_decode_gain import _old_bits
from test_gpu_window_decode_half import _block_size_for, _signal
from test_gpu_window_decode_mixed import _compare, _decode_plan_rows
from test_gpu_window_decode_placed import SNAN, Tables, _assert_span_kinds, _i64, _old_with_nans
from window_half_oracle import half_bits_of_float32
from window_oracle import window_expected
from window_stats_oracle import stats_of_rows, window_counts

pytestmark = pytest.mark.gpu

U64 = 1 << 64
CANARY = 0x5A5A
GUARD = 32  # int16 elements: 64 bytes in front of and behind the rows
REC_PATTERN = -0x0123456789ABCDEF
CUT = 3     # the stream whose image loses bytes of its last block
ROW_NAMES = ("int16", "float32", "float16", "bfloat16")
WITNESS_SHIFTS = 5  # a placed run puts witness window i at o = 1 + i % 5


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


# ---- the cases, on the CPU ---------------------------------------------------------------------------------------------------------
# kind: "same" / "mixed" / "mix"; channels: the rows of a window; variants: key -> its streams; witness_stream: key -> the stream
# its witnesses sit on; candidates / scales: per variant the window the witnesses were searched on and 2^15 or - a down-mix - 2^16;
# rows16 / rows32: the oracle's rows of every window; olds: (window, row, t, old) of the "fused" witnesses
Case = collections.namedtuple("Case", "kind images headers decoded lengths spbs channels frames windows gains spans n_plain "
                                      "variants witness_stream candidates scales witnesses olds rows16 rows32")


@functools.lru_cache(maxsize=None)
def _mbs(channels, bits, target):
    return _block_size_for(channels, bits, target)


def _corpus(formats, seed):
    """formats: [(channels, bits, M/S, the spb to stay under)] -> images of about 2.5 blocks (stream CUT: truncated inside its last
    block), the oracle's decodes, lengths, headers"""
    images, decoded, lengths = [], [], []
    for i, (ch, bits, ms, target) in enumerate(formats):
        mbs = _mbs(ch, bits, target)
        rc, block_size, spb = ob.geometry(mbs, ch, bits)
        assert rc == 0 and 48 <= spb <= 160, (ch, bits, target, spb)  # at least two whole 16-sample chunks a block
        n = (2 * spb + spb // 2, 2 * spb + spb // 2 + 7, 3 * spb - 1, 2 * spb + spb // 2 + 1, 2 * spb + 21)[i % 5]
        img = ob.encode(_signal(n, ch, (3500, 3900, 1700, 12000)[i % 4], seed + i), bits, mbs, 48000, ms, 0)
        if i == CUT:
            payload = len(img) - 31
            last = payload - (-(-payload // block_size) - 1) * block_size
            cut = (last - 18 * ch) // 2
            assert cut >= 1 and payload > 2 * block_size  # inside the coded bytes of the third block
            img = img[:len(img) - cut]
        images.append(img)
        decoded.append(ob.decode(img)[0])
        lengths.append(n)
    headers = [parse_header(img[:31]) for img in images]
    assert [h.num_samples for h in headers] == lengths and len(set(lengths)) >= min(len(lengths), 4)  # ragged
    return images, decoded, lengths, headers


def _variant(kind, h):
    ms = int(h.num_channels == 2 and h.ch_process_method == 1)
    return (h.num_channels, h.bits_per_sample, ms) if kind == "mix" else (h.bits_per_sample, ms)


def _plain_windows(lengths, spbs, frames):
    """per stream: phase 0, phase 3, phase spb - 1, the window that ends at the stream's end, the one that starts on its last
    frame; then one past the end and two stray ones"""
    rows = []
    for s, (n, spb) in enumerate(zip(lengths, spbs)):
        rows += [(s, spb * (s % 2)), (s, spb * ((s + 1) % 2) + 3), (s, spb - 1), (s, max(n - frames, 0)), (s, n - 1)]
    rows += [(0, lengths[0]), (len(lengths), 0), (-1, 5)]
    return np.array(rows, dtype=np.int64)


def _plain_spans(n, frames, smin):
    """(T, 0); an empty span; o > 0 odd with L so short that lanes k >= 1 only fill; o >= T; spans that run past the row and - on
    the windows at a stream's end - past num_samples"""
    t = frames
    kinds = [(t, 0), (0, 0), (7, 3), (1, t), (U64 - 1, 1), (5, t - 1), (2, 5), (16, 1), (smin + 1, 3), (40, t - 30), (16, 7), (3, 1 << 63)]
    return _i64([kinds[j % len(kinds)] for j in range(n)])  # twelve kinds over five windows a stream: every pairing in turn


def _plain_gains(n, seed):
    gains = np.random.default_rng(seed).uniform(-2.0, 2.0, size=n).astype(np.float32)
    gains[:6] = [1.0, -1.0, 0.0, 2.0 ** -120, -2.0 ** -136, -0.0]
    gains[6::7] = -1.5
    return gains


@functools.lru_cache(maxsize=None)
def matrix_case(kind, key):
    """kind "same": key a geometry of wm.GEOMETRIES; "mixed": a name of wm.MIXED_PLANS; "mix": out_channels.  Everything a case
    runs and expects, from the oracles alone - no device, so the host test confirms the same witnesses"""
    if kind == "same":
        ch, bits, ms = key
        formats = [(ch, bits, ms, 70 + 20 * bits)] * 5
        seed, channels = 21000 + 100 * ch + 10 * bits + int(ms), ch
    elif kind == "mixed":
        ch, variants = wm.MIXED_PLANS[key]
        if ch == 2:
            formats = [(2, 4, False, 128), (2, 3, True, 64), (2, 2, False, 128), (2, 4, True, 64), (2, 3, False, 128), (2, 2, True, 64),
                       (2, 4, False, 64), (2, 3, True, 128), (2, 4, True, 128)]
        else:
            formats = [(ch, 4, False, 128), (ch, 3, False, 64), (ch, 2, False, 128), (ch, 4, False, 128), (ch, 3, False, 64)]
        assert {(b, ms) for _, b, ms, _ in formats} == set(variants)
        seed, channels = 22000 + 100 * ch, ch
    else:
        formats = [(1, 4, False, 128), (2, 4, False, 64), (2, 3, True, 128), (1, 2, False, 64), (2, 2, False, 128), (1, 3, False, 64),
                   (2, 4, True, 128), (2, 3, False, 64), (2, 2, True, 128), (1, 2, False, 128)]
        assert {(c, b, ms) for c, b, ms, _ in formats} == set(wm.CHANNEL_VARIANTS)
        seed, channels = 23000, int(key)
    images, decoded, lengths, headers = _corpus(formats, seed)
    spbs = [h.num_samples_per_block for h in headers]
    frames = (3 * max(spbs)) // 2 | 1
    assert frames < 250
    expect = (lambda w, dtype: channel_mix_expected(decoded, w, frames, channels, dtype)) if kind == "mix" else \
             (lambda w, dtype: window_expected(decoded, w, frames, channels, dtype))
    variants = collections.OrderedDict()
    for s, h in enumerate(headers):
        variants.setdefault(_variant(kind, h), []).append(s)
    if kind != "same":
        assert len({h.block_size for h in headers}) >= 2
        blocks = {-(-(frames - 1) // min(spbs[s] for s in streams)) + 1 for streams in variants.values()}
        assert len(blocks) >= 2, blocks  # K = ceil((T - 1) / spb) + 1 of the variant's smallest block: it differs between launches

    plain = _plain_windows(lengths, spbs, frames)
    plain_spans = _plain_spans(len(plain), frames, min(spbs))
    _assert_span_kinds(plain, plain_spans, lengths, spbs, frames)

    # one candidate window per variant: on block 0 or 1 of a stream that is whole; both blocks are complete, inside num_samples,
    # and followed by the header of another block, so the wide code loads of all their chunks stay inside the stream's bytes
    witness_stream, candidates = {}, []
    for i, (v, streams) in enumerate(variants.items()):
        s = [s for s in streams if s != CUT][0]
        assert 2 * spbs[s] + 18 <= lengths[s]
        witness_stream[v] = s
        candidates.append((s, (i % 2) * spbs[s]))
    candidates = np.array(candidates, dtype=np.int64)
    cand_spbs = [spbs[s] for s in candidates[:, 0]]
    twins = [kind == "mix" and channels == 2 and headers[s].num_channels == 1 for s in candidates[:, 0]]
    scales = [65536.0 if kind == "mix" and channels == 1 and headers[s].num_channels == 2 else 32768.0 for s in candidates[:, 0]]
    # Le of a witness window in the placed run is at least T - WITNESS_SHIFTS: the chunks of the block are the same
    witnesses = go.vector_witnesses(expect(candidates, np.float32), candidates, cand_spbs, les=[frames - WITNESS_SHIFTS] * len(candidates),
                                    scale=scales, twins=twins)
    assert len(witnesses) == 16 * len(variants)
    windows = np.concatenate([plain, candidates[[w.window for w in witnesses]]])
    gains = np.concatenate([_plain_gains(len(plain), seed), np.array([w.gain for w in witnesses], dtype=np.float32)])
    shifts = 1 + np.arange(len(witnesses)) % WITNESS_SHIFTS
    spans = np.concatenate([plain_spans, np.stack([frames - shifts, shifts], axis=1).astype(np.int64)])
    olds = [(len(plain) + i, row, w.t, old) for i, w in enumerate(witnesses) if w.olds for row, old in w.olds]
    return Case(kind, images, headers, decoded, lengths, spbs, channels, frames, windows, gains, spans, len(plain), variants,
                witness_stream, candidates, scales, witnesses, olds, expect(windows, np.int16), expect(windows, np.float32))


# ---- runs between canaries ---------------------------------------------------------------------------------------------------------
def _torch_dtype(torch, name):
    return torch.int16 if name == "int16" else go.torch_dtype(name)


def _buffer(torch, shape, name, old_bits=None):
    width = 2 if name == "float32" else 1  # int16 elements per row element
    size = int(np.prod(shape)) * width
    big = torch.full((size + 2 * GUARD,), CANARY, dtype=torch.int16, device="cuda")
    out = big[GUARD:GUARD + size].view(_torch_dtype(torch, name)).view(*shape)
    if old_bits is not None:
        bits = np.ascontiguousarray(old_bits)
        big[GUARD:GUARD + size].copy_(torch.from_numpy(bits.view(np.int16).reshape(-1)))  # bits, NaNs included
    return big, out


def _rows_of(big, shape, name):
    host = big.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), "wrote outside its rows"
    return host[GUARD:-GUARD].view(np.uint32 if name == "float32" else np.uint16).reshape(shape)


def _plain_want(case, name):
    if name == "int16":
        return case.rows16.view(np.uint16)
    if name == "float32":
        return case.rows32.view(np.uint32)
    return half_bits_of_float32(case.rows32, name)


def _assert_every_variant_works(case, want, label):
    """every variant has a window on one of its streams, inside the stream, whose expected rows are not zero: the kernel of that
    variant has something to be wrong about"""
    busy = want.reshape(len(want), -1).any(axis=1)
    for v, streams in case.variants.items():
        on = [w for w, (s, f) in enumerate(case.windows.tolist()) if s in streams and 0 <= f < case.lengths[s] and busy[w]]
        assert on, (label, "no work for variant", v)


def _assert_witnesses_ride(case):
    """the gain and placed runs carry four witnesses of each kind for every variant, on a stream of that variant"""
    seen = collections.Counter()
    for i, w in enumerate(case.witnesses):
        s, first = case.windows[case.n_plain + i].tolist()
        v = _variant(case.kind, case.headers[s])
        assert case.witness_stream[v] == s and first % case.spbs[s] == 0 and case.gains[case.n_plain + i] == w.gain
        assert case.rows32[case.n_plain + i, w.channel, w.t] != 0
        seen[(v, w.kind)] += 1
    assert seen == {(v, k): 4 for v in case.variants for k in go.VECTOR_KINDS}, seen


def _assert_witnesses_bite(case, name, placed, want, old, label):
    """the expected rows of a run hold, at every witness element of the run's type, other bits than the implementation the witness
    is against would give: the float64 product rounded once to float16 / bfloat16 (STORE), old + g * f rounded once to float32
    (ADD), the gain applied to the integer sample before the scale (STORE, float32).  Values are compared: every one is finite."""
    value = lambda bits: float(go.from_bits(np.array([bits], dtype=want.dtype), name).double().item())
    bitten = collections.Counter()
    for i, w in enumerate(case.witnesses):
        k = case.n_plain + i
        at = (int(case.spans[k, 1]) if placed else 0) + w.t
        g, f = float(w.gain), float(case.rows32[k, w.channel, w.t])
        if old is None and w.kind == "double_" + name:
            wrong = float(go.round_f64(g * f, name))
        elif old is None and w.kind == "order" and name == "float32":
            scale = np.float32(case.scales[w.window])
            s = np.float32(f * float(scale))  # the integer the decoder holds: the sample, or L + R of a down-mix
            assert float(s) == int(s) and float(s) / float(scale) == f
            wrong = float(np.float32(s * w.gain) / scale)  # float32 arithmetic: two roundings
        elif old is not None and w.kind == "fused" and name == "float32":
            for row, _ in w.olds:
                planted = value(old[k, row, at])
                assert value(want[k, row, at]) != float(np.float32(planted + g * f)), (label, "fused", i, w)
            bitten[w.kind] += 1
            continue
        else:
            continue
        assert value(want[k, w.channel, at]) != wrong, (label, w.kind, i, w)
        bitten[w.kind] += 1
    kinds = (["fused"] if name == "float32" else []) if old is not None else (["order"] if name == "float32" else ["double_" + name])
    assert bitten == {kind: 4 * len(case.variants) for kind in kinds}, (label, bitten)


def _check_case(engine, case, make_plan, label):
    import torch
    flat, table = _pack(case.images)
    d_img = torch.from_numpy(flat).cuda()
    for got, want in zip(_decode_plan_rows(engine, torch, case.headers, table, d_img), case.decoded):  # D_s of the definition
        assert np.array_equal(got, want), (label, "AADHip_DecodePlanRun and the oracle's decode differ")
    n, channels, frames = case.rows16.shape
    shape = (n, channels, frames)
    windows = case.windows
    tables = Tables(torch, windows, case.spans, case.gains)
    plan = make_plan(table)
    try:
        # AADHip_WindowDecodePlanRun and ...RunStats
        stats_want = stats_of_rows(case.rows16, window_counts(case.lengths, windows, frames))
        _assert_every_variant_works(case, case.rows16, label)
        _assert_every_variant_works(case, stats_want[..., 1], label + ("statistics",))
        for name in ROW_NAMES:
            dtype, want = _torch_dtype(torch, name), _plain_want(case, name)
            _assert_every_variant_works(case, want, label + (name,))
            big, out = _buffer(torch, shape, name)
            assert plan.run(d_img, tables.windows, frames, dtype, out=out).data_ptr() == out.data_ptr()
            _compare(_rows_of(big, shape, name), want, label + (name, "rows"), windows)
            big, out = _buffer(torch, shape, name)
            whole = torch.full((n * channels * 4 + 16,), REC_PATTERN, dtype=torch.int64, device="cuda")
            plan.run(d_img, tables.windows, frames, dtype, out=out, stats=whole[8:-8].view(n, channels, 4))
            _compare(_rows_of(big, shape, name), want, label + (name, "rows of the statistics run"), windows)
            for rows in (True, False):
                if not rows:
                    whole.fill_(REC_PATTERN)
                    assert plan.run(d_img, tables.windows, frames, dtype, stats=whole[8:-8].view(n, channels, 4), rows=False) is not None
                host = whole.cpu().numpy()
                assert (host[:8] == REC_PATTERN).all() and (host[-8:] == REC_PATTERN).all(), (label, name, "wrote outside its records")
                got = host[8:-8].reshape(n, channels, 4)
                assert np.array_equal(got, stats_want), (label, name, "statistics", rows, np.argwhere(got != stats_want)[:3].tolist())
        # AADHip_WindowDecodePlanRunGain and ...RunPlaced
        _assert_witnesses_ride(case)
        rng = np.random.default_rng(len(windows))
        for name in go.DTYPES:
            dtype = go.torch_dtype(name)
            value = lambda old: go.bits_of(torch.tensor([old], dtype=torch.float32).to(dtype))[0]
            for placed in (False, True):
                spans = case.spans if placed else None
                run = lambda out, add: plan.run(d_img, tables.windows, frames, dtype, out=out, gain=tables.gains, accumulate=add,
                                                spans=tables.spans if placed else None)
                what = label + (name, "placed" if placed else "gain")
                want = po.placed_expected(case.rows32, spans, case.gains, name)
                if not placed:
                    assert np.array_equal(want, go.gain_expected(case.rows32, case.gains, name))
                _assert_every_variant_works(case, want, what)
                _assert_witnesses_bite(case, name, placed, want, None, what)
                big, out = _buffer(torch, shape, name)
                run(out, False)
                _compare(_rows_of(big, shape, name), want, what + ("STORE",), windows)
                old = _old_with_nans(rng, shape, name, spans) if placed else _old_bits(rng, shape, name)
                for w, row, t, v in case.olds:
                    o = int(case.spans[w, 1]) if placed else 0
                    assert po.clipped(case.spans[w:w + 1], 1, frames)[0][0] > t
                    old[w, row, o + t] = value(v)
                want = po.placed_expected(case.rows32, spans, case.gains, name, old)
                _assert_witnesses_bite(case, name, placed, want, old, what)
                big, out = _buffer(torch, shape, name, old)
                run(out, True)
                got = _rows_of(big, shape, name)
                _compare(got, want, what + ("ADD",), windows)
                if placed:
                    quiet, loud = SNAN[name]
                    assert ((got == quiet) | (got == loud)).sum() == ((old == quiet) | (old == loud)).sum() > 0  # every NaN came back
        # AADHip_WindowDecodePlanRunPlacedStats
        want = po.placed_stats_expected(case.rows16, case.lengths, windows, case.spans)
        _assert_every_variant_works(case, want[..., 1], label + ("placed statistics",))
        whole = torch.full((n * channels * 4 + 16,), REC_PATTERN, dtype=torch.int64, device="cuda")
        plan.run(d_img, tables.windows, frames, stats=whole[8:-8].view(n, channels, 4), rows=False, spans=tables.spans)
        host = whole.cpu().numpy()
        assert (host[:8] == REC_PATTERN).all() and (host[-8:] == REC_PATTERN).all(), (label, "wrote outside its records")
        got = host[8:-8].reshape(n, channels, 4)
        assert np.array_equal(got, want), (label, "placed statistics", np.argwhere(got != want)[:3].tolist())
        torch.cuda.synchronize()
        tables.assert_unchanged(label)
    finally:
        plan.close()
    assert torch.equal(d_img.cpu(), torch.from_numpy(flat)), "the images changed"


# ---- the matrix cases: tests/window_matrix.py names them ---------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", wm.GEOMETRIES, ids=wm.geometry_id)
def test_same_format_plans(engine, geometry):
    case = matrix_case("same", geometry)
    assert len(case.variants) == 1 and len(case.windows) == 5 * 5 + 3 + 16
    _check_case(engine, case, lambda table: engine.window_decode_plan(case.headers[0], table, True), (geometry,))


@pytest.mark.parametrize("plan", list(wm.MIXED_PLANS), ids=str)
def test_mixed_plans(engine, plan):
    channels, variants = wm.MIXED_PLANS[plan]
    case = matrix_case("mixed", plan)
    assert len({(h.bits_per_sample, h.ch_process_method) for h in case.headers}) == len(variants) == len(case.variants)
    assert {h.num_channels for h in case.headers} == {channels}
    _check_case(engine, case, lambda table: engine.mixed_window_decode_plan(case.headers, table, True), ("mixed", plan))


@pytest.mark.parametrize("out_channels", wm.OUT_CHANNELS, ids=wm.out_channels_id)
def test_channel_mix_plans(engine, out_channels):
    case = matrix_case("mix", out_channels)
    assert len({(h.num_channels, h.bits_per_sample, h.ch_process_method) for h in case.headers}) == 9 == len(case.variants)
    if out_channels == 1:  # the half step of the down-mix is there: a float32 row that is not the int16 floor mix / 32768
        assert (case.rows32 != case.rows16.astype(np.float32) / np.float32(32768.0)).sum() > 100
    _check_case(engine, case, lambda table: engine.channel_mix_window_decode_plan(case.headers, table, out_channels, True),
                ("channel mix", out_channels))
