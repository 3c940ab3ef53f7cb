"""Window decode with a span per window (AADHip_WindowDecodePlanRunPlaced / ...RunPlacedStats, include/aad_hip.h;
aad_amd/csrc/aad_decode_window_placed.hip.h).

Bar: every row EQUALS, as bit patterns, the torch expression of the definition on the CPU (tests/window_placed_oracle.py over
tests/window_oracle.py, tests/channel_mix_oracle.py and tests/window_gain_oracle.py), into a buffer with 64 canary bytes on both
sides; the window, span and gain tables lie between canaries too and come back unchanged.  STORE runs go into rows that hold the
canary pattern, so an element nobody wrote shows; ADD runs go into random finite values of the type (-0, subnormals among them)
with signalling-NaN bit patterns planted outside the spans, which must come back bit for bit.
  1. all variants: same-format plans (bits 2 / 3 / 4 x mono, stereo, mid/side, 3 channels), a mixed plan of several variants and
     two block sizes, channel-mix plans in both directions; float32, float16, bfloat16; STORE and ADD; streams of about 2.5 blocks
     at max_block_size 128 and T = 2 spb + 3, the plan (K = 4 lanes a row) asserted from the policy header first;
  2. the gain oracle's witnesses with every witness window shifted to a non-zero o: the two roundings hold through the placed kernels;
  3. NULL spans and (T, 0) spans: AADHip_WindowDecodePlanRunGain's bytes;
  4. the placed statistics against the oracle's sums over Le, and with NULL spans against AADHip_WindowDecodePlanRunStats without rows;
  5. Engine.mix_windows(noise_spans=...) against its two-run definition;
  6. errors through the C call, the unaligned span table among them; a refused run leaves `out` untouched;
  7. AADHip_ContextSignalNextRun around a placed run of several kernels;
  8. past the grid cap, with spans that leave most lanes nothing but their fill."""
import numpy as np
import pytest

import oracle_binding as ob
import window_gain_oracle as go
import window_placed_oracle as po
from aad_amd.capi import AADApiResult, SAMPLE_FLOAT16, SAMPLE_FLOAT32, SAMPLE_INT16
from aad_amd.engine import parse_header, snr_gains
from channel_mix_oracle import channel_mix_expected
from test_gpu_chip_filling_paths import (MAX_GRID, P, chip, encoded_streams, pack_images, policy, spb_of, variant_launches,  # noqa: F401
                                         window_launch, window_tile)
from test_gpu_window_decode import _pack
from test_gpu_window_decode_gain import (CANARY, GUARD, KINDS, _assert_witnesses_present, _gains_and_windows, _old_bits, _plain_corpus,
                                         _plans, witness)  # noqa: F401
from test_gpu_window_decode_half import _channel_corpus, _corpus_windows, _mixed_corpus, _plain_windows, _signal
from test_gpu_window_decode_mixed import _compare, _decode_plan_rows
from window_oracle import window_expected
from window_stats_oracle import channel_mix_stats_expected

pytestmark = pytest.mark.gpu

U64 = 1 << 64
SNAN = {"float32": (0x7F800001, 0xFFA00000), "float16": (0x7C01, 0xFD55), "bfloat16": (0x7F81, 0xFFA0)}  # quiet bit clear


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _i64(rows):
    """python ints of any sign and size below 2^64 -> int64 array (values wrap)"""
    return np.array([[int(v) % U64 for v in r] for r in rows], dtype=np.uint64).view(np.int64)


class Tables:
    """the window, span and gain tables of a run on the device, each with 64 canary bytes in front of it and behind it"""

    def __init__(self, torch, windows, spans, gains):
        self.torch, self.whole, self.snapshot = torch, [], []
        self.windows = self._place(np.ascontiguousarray(windows, dtype=np.int64), torch.int64)
        self.spans = None if spans is None else self._place(np.ascontiguousarray(spans, dtype=np.int64), torch.int64)
        self.gains = None if gains is None else self._place(np.ascontiguousarray(gains, dtype=np.float32), torch.float32)

    def _place(self, array, dtype):
        torch = self.torch
        guard = 64 // array.itemsize
        host = np.frombuffer(b"\x5A" * 64, dtype=array.dtype)
        assert len(host) == guard
        whole = torch.from_numpy(np.concatenate([host, array.reshape(-1), host])).cuda()
        self.whole.append(whole)
        self.snapshot.append(whole.cpu())
        return whole[guard:guard + array.size].view(array.shape)

    def assert_unchanged(self, label):
        for whole, before in zip(self.whole, self.snapshot):
            assert self.torch.equal(whole.cpu().view(self.torch.uint8), before.view(self.torch.uint8)), (label, "a table changed")


def _out_buffer(torch, n, channels, frames, name, old_bits):
    count = n * channels * frames
    width = 2 if name == "float32" else 1  # int16 elements per row element
    big = torch.full((count * width + 2 * GUARD,), CANARY, dtype=torch.int16, device="cuda")
    out = big[GUARD:GUARD + count * width].view(go.torch_dtype(name)).view(n, channels, frames)
    if old_bits is not None:
        out.view(torch.int32 if name == "float32" else torch.int16).copy_(
            torch.from_numpy(np.ascontiguousarray(old_bits).view(np.int32 if name == "float32" else np.int16)))  # bits, NaNs included
    return big, out, count * width


def _rows_of(big, n, channels, frames, name, size):
    host = big.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[GUARD + size:] == CANARY).all(), "wrote outside its rows"
    return host[GUARD:GUARD + size].view(np.uint32 if name == "float32" else np.uint16).reshape(n, channels, frames)


def _run_placed(torch, plan, d_img, tables, frames, channels, name, old_bits=None, label=()):
    """a run with spans into `out=` between 64-byte canaries -> the rows' bit patterns; old_bits: an ADD run over them"""
    n = len(tables.windows)
    big, out, size = _out_buffer(torch, n, channels, frames, name, old_bits)
    got = plan.run(d_img, tables.windows, frames, go.torch_dtype(name), out=out, gain=tables.gains, accumulate=old_bits is not None,
                   spans=tables.spans)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    tables.assert_unchanged(label)
    return _rows_of(big, n, channels, frames, name, size)


def _old_with_nans(rng, shape, name, spans):
    """the gain test's old rows, with signalling NaNs outside the spans: next to both ends of every span and on every third element"""
    old = _old_bits(rng, shape, name)
    n, _, frames = shape
    quiet, loud = SNAN[name]
    for w, (le, o) in enumerate(po.clipped(spans, n, frames)):
        outside = np.ones(frames, dtype=bool)
        outside[o:o + le] = False
        plant = outside & ((np.arange(frames) + w) % 3 == 0)
        for t in (o - 1, o + le):
            if le and 0 <= t < frames:
                plant[t] = True
        old[w][:, plant] = quiet if w % 2 else loud
    return old


def _check_all(torch, plan, d_img, windows, spans, gains, rows32, channels, label, seed, olds=()):
    """STORE and ADD of every type against the oracle"""
    rng = np.random.default_rng(seed)
    frames = rows32.shape[2]
    tables = Tables(torch, windows, spans, gains)
    for name in go.DTYPES:
        got = _run_placed(torch, plan, d_img, tables, frames, channels, name, label=label)
        _compare(got, po.placed_expected(rows32, spans, gains, name), label + (name, "STORE"), windows)
        old = _old_with_nans(rng, rows32.shape, name, spans)
        for w, t, value in olds:
            old[w, :, t] = go.bits_of(torch.tensor([value], dtype=torch.float32).to(go.torch_dtype(name)))[0]
        got = _run_placed(torch, plan, d_img, tables, frames, channels, name, old_bits=old, label=label)
        want = po.placed_expected(rows32, spans, gains, name, old)
        _compare(got, want, label + (name, "ADD"), windows)
        quiet, loud = SNAN[name]
        assert ((got == quiet) | (got == loud)).sum() == ((old == quiet) | (old == loud)).sum() > 0  # every NaN came back


# ---- the corpus, the windows and the spans -----------------------------------------------------------------------------------------
MBS = 128
CUT = 3  # the stream whose image loses its last bytes


def _streams(formats, seed):
    """formats: [(channels, bits, M/S, max_block_size)] -> images of about 2.5 blocks each (stream CUT: truncated inside its last
    block), the oracle's decodes, lengths, headers"""
    images, decoded, lengths = [], [], []
    for i, (ch, bits, ms, mbs) in enumerate(formats):
        block_size, spb = spb_of(ch, bits, mbs)
        n = (2 * spb + spb // 2, 2 * spb + spb // 2 + 7, 3 * spb - 1, 2 * spb + spb // 2 + 1, 2 * spb + 1)[i % 5]
        img = ob.encode(_signal(n, ch, (3500, 3900, 700, 12000)[i % 4], seed + i), bits, mbs, 48000, ms, 0)
        if i == CUT:
            last = (len(img) - 31) - ((len(img) - 31 - 1) // block_size) * block_size
            assert last > 18 * ch + 7
            img = img[:-7]
        images.append(img)
        decoded.append(ob.decode(img)[0])
        lengths.append(n)
    headers = [parse_header(img[:31]) for img in images]
    assert [h.num_samples for h in headers] == lengths
    return images, decoded, lengths, headers


def _cases(lengths, spbs, frames):
    """-> (windows int64 [N, 2], spans int64 [N, 2]): the issue's list of spans, each over starts at phase 0, 3 and spb - 1, on a
    stray stream and at the end of the truncated image; crops that run past num_samples; spans so short that lanes k >= 1 only fill"""
    t, smin = frames, min(spbs)
    spans = [(t, 0), (0, 0), (5, t - 1), (1, t), (U64 - 1, 1), (3, 1 << 63), (16, 0), (16, 1), (16, 7), (smin + 1, 3), (2, 5)]
    rows = []
    for j, (length, o) in enumerate(spans):
        for s, phase in ((0, 0), (1, 3), (2, spbs[2] - 1)):
            rows.append((s, spbs[s] * (j % 2) + phase, length, o))
        rows.append((len(lengths), j, length, o))                           # a stray stream
        rows.append((CUT, max(lengths[CUT] - 20 - 3 * j, 0), length, o))    # the truncated image's last frames
    rows += [(0, lengths[0] - 3, 10, 2), (1, lengths[1] - 1, t, 4), (2, lengths[2], 8, 1), (1, -1, 8, 1), (4, lengths[4] - 17, 40, t - 30)]
    rows += [(0, 0, 2, 5), (1, spbs[1], 1, t - 1), (4, 2 * spbs[4], 3, 0), (-1, 0, t, 0)]
    table = _i64(rows)
    return np.ascontiguousarray(table[:, :2]), np.ascontiguousarray(table[:, 2:])


def _gains(n, seed):
    gains = np.random.default_rng(seed).uniform(-2.0, 2.0, size=n).astype(np.float32)
    gains[:6] = [1.0, -1.0, 0.0, 2.0 ** -120, -2.0 ** -136, -0.0]
    gains[6::7] = -1.5  # negative gains over every kind of span: no -0 may show outside one
    return gains


def _assert_span_kinds(windows, spans, lengths, spbs, frames):
    """the case list holds what it claims"""
    clipped = po.clipped(spans, len(spans), frames)
    assert {le for le, _ in clipped} >= {0, 1, 2, 16, frames - 1, frames}
    assert any(o % 2 == 1 and le for le, o in clipped) and any(o == frames - 1 for _, o in clipped)
    phases, past, fill_only = set(), 0, 0
    for (s, f), (le, _) in zip(windows.tolist(), clipped):
        if 0 <= s < len(lengths) and 0 <= f < lengths[s]:
            phases.add(-1 if f % spbs[s] == spbs[s] - 1 else f % spbs[s])
            past += le > lengths[s] - f
            fill_only += 0 < le + f % spbs[s] <= spbs[s]  # lanes k >= 1 leave before they decode
    assert {0, 3, -1} <= phases and past >= 3 and fill_only >= 3


# ---- 1. all variants ---------------------------------------------------------------------------------------------------------------
PLAIN = [(c, b, ms) for c, ms in ((1, False), (2, False), (2, True), (3, False)) for b in (4, 3, 2)]


@pytest.mark.parametrize("geometry", PLAIN, ids=lambda g: "%dch%db%s" % (g[0], g[1], "ms" if g[2] else ""))
def test_same_format_plans(engine, policy, chip, geometry):
    import torch
    channels, bits, ms = geometry
    _, spb = spb_of(channels, bits, MBS)
    images, decoded, lengths, headers = _streams([(channels, bits, ms, MBS)] * 5, 11000 + 100 * channels + 10 * bits + int(ms))
    frames = 2 * spb + 3
    windows, spans = _cases(lengths, [spb] * 5, frames)
    _assert_span_kinds(windows, spans, lengths, [spb] * 5, frames)
    n = len(windows)
    launch = window_launch(policy, chip, n, frames, channels, bits, spb)
    assert launch.ok == 1 and launch.blocks_per_window == 4 and launch.lanes == n * 4 * channels and launch.grid >= 2, launch
    flat, table = _pack(images)
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.window_decode_plan(headers[0], table, True)
    try:
        rows32 = window_expected(decoded, windows, frames, channels, np.float32)
        _check_all(torch, plan, d_img, windows, spans, _gains(n, bits), rows32, channels, (geometry,), 70 + bits)
    finally:
        plan.close()
    assert torch.equal(d_img.cpu(), torch.from_numpy(flat)), "the images changed"


MIXED = [(2, 4, False, 128), (2, 3, True, 128), (2, 4, False, 64), (2, 2, True, 128), (2, 3, True, 64)]
CHANNEL = [(1, 4, False, 128), (2, 4, False, 128), (2, 3, True, 64), (1, 2, False, 64), (2, 2, False, 128)]


def _assert_variant_plans(policy, chip, headers, n, frames, at_least):
    launches = variant_launches(policy, chip, headers, n, frames)
    assert len(launches) >= at_least and len({h.block_size for h in headers}) >= 2
    for key, launch in launches.items():
        assert launch.ok == 1 and launch.blocks_per_window >= 4 and launch.lanes == n * launch.blocks_per_window * key[0], (key, launch)
    assert len({launch.blocks_per_window for launch in launches.values()}) >= 2  # K differs between the launches


def test_mixed_plan(engine, policy, chip):
    import torch
    images, decoded, lengths, headers = _streams(MIXED, 12000)
    spbs = [h.num_samples_per_block for h in headers]
    frames = 2 * max(spbs) + 3
    windows, spans = _cases(lengths, spbs, frames)
    _assert_span_kinds(windows, spans, lengths, spbs, frames)
    _assert_variant_plans(policy, chip, headers, len(windows), frames, 3)
    flat, table = _pack(images)
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)
    try:
        rows32 = window_expected(decoded, windows, frames, 2, np.float32)
        _check_all(torch, plan, d_img, windows, spans, _gains(len(windows), 12), rows32, 2, ("mixed",), 81)
    finally:
        plan.close()


@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_channel_mix_plans(engine, policy, chip, out_channels):
    """to_mono: the R lane of a pair fills nothing; to_stereo: a mono source fills and stores both rows"""
    import torch
    images, decoded, lengths, headers = _streams(CHANNEL, 13000)
    spbs = [h.num_samples_per_block for h in headers]
    frames = 2 * max(spbs) + 3
    windows, spans = _cases(lengths, spbs, frames)
    _assert_span_kinds(windows, spans, lengths, spbs, frames)
    _assert_variant_plans(policy, chip, headers, len(windows), frames, 4)
    flat, table = _pack(images)
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    try:
        rows32 = channel_mix_expected(decoded, windows, frames, out_channels, np.float32)
        _check_all(torch, plan, d_img, windows, spans, _gains(len(windows), 13), rows32, out_channels, ("channel mix", out_channels), 91)
    finally:
        plan.close()


# ---- 2. the witnesses, shifted -------------------------------------------------------------------------------------------------------
def test_witnesses_at_a_non_zero_offset(engine, witness):
    """the gain test's witness windows - a product that rounds otherwise when its float32 rounding is skipped, an old value that
    gives another float32 under an fma, a subnormal product - each placed at o = 1 + w % 5 > 0, the old values planted o further on"""
    import torch
    channels, bits, ms = 2, 4, True
    images, hd = _plain_corpus(channels, bits, ms)
    spb = hd.num_samples_per_block
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    d_img = torch.from_numpy(flat).cuda()
    decoded = _decode_plan_rows(engine, torch, [hd] * len(images), table, d_img)
    frames = (3 * spb) // 2 | 1
    plain = _plain_windows(lengths, spb, frames)
    windows, gains, olds = _gains_and_windows(plain, 5, spb, 104)
    rows32 = window_expected(decoded, windows, frames, channels, np.float32)
    _assert_witnesses_present(rows32, windows, gains, olds, witness, len(plain))
    offsets = 1 + np.arange(len(windows)) % 5
    spans = np.stack([frames - offsets - (np.arange(len(windows)) % 3), offsets], axis=1).astype(np.int64)
    assert (spans[:, 1] > 0).all() and (spans[:, 0] > 8).all()
    shifted = [(w, t + int(offsets[w]), old) for w, t, old in olds]
    plan = engine.window_decode_plan(hd, table, True)
    try:
        _check_all(torch, plan, d_img, windows, spans, gains, rows32, channels, ("witnesses",), 17, olds=shifted)
    finally:
        plan.close()


# ---- 3. NULL spans and (T, 0) spans ----------------------------------------------------------------------------------------------------
def test_null_and_full_spans_are_the_gain_run(engine):
    import torch
    lib = engine.lib
    for label, plan, channels, flat, table, spbs in _plans(engine):
        try:
            d_img = torch.from_numpy(flat).cuda()
            lengths = [int(n) for n in table["num_samples"]]
            frames = 141
            windows = _corpus_windows(lengths, spbs, frames)
            n = len(windows)
            full = np.tile(np.array([[frames, 0]], dtype=np.int64), (n, 1))
            full[1::2, 0] = np.array([frames + 1, -1, 1 << 62] * n, dtype=np.int64)[:len(full[1::2])]  # any L >= T is T
            tables = Tables(torch, windows, full, _gains(n, 3))
            rng = np.random.default_rng(33)
            for name in go.DTYPES:
                for add in (False, True):
                    old = _old_bits(rng, (n, channels, frames), name) if add else None

                    def run(call):
                        big, out, size = _out_buffer(torch, n, channels, frames, name, old)
                        torch.cuda.synchronize()  # a direct C call is not ordered against torch's stream
                        assert call(out) == AADApiResult.OK, engine.last_error()
                        torch.cuda.synchronize()
                        return _rows_of(big, n, channels, frames, name, size)

                    common = (plan.handle, d_img.data_ptr(), n, tables.windows.data_ptr())
                    rest = lambda out: (frames, KINDS[name], out.data_ptr(), tables.gains.data_ptr(), int(add))
                    want = run(lambda out: lib.AADHip_WindowDecodePlanRunGain(*common, *rest(out)))
                    assert (want != (CANARY | CANARY << 16 if name == "float32" else CANARY)).any()
                    null = run(lambda out: lib.AADHip_WindowDecodePlanRunPlaced(*common, None, *rest(out)))
                    assert null.tobytes() == want.tobytes(), (label, name, add, "NULL spans")
                    whole = run(lambda out: lib.AADHip_WindowDecodePlanRunPlaced(*common, tables.spans.data_ptr(), *rest(out)))
                    assert whole.tobytes() == want.tobytes(), (label, name, add, "(T, 0) spans")
            tables.assert_unchanged(label)
        finally:
            plan.close()


# ---- 4. the statistics -----------------------------------------------------------------------------------------------------------------
REC_PATTERN = -0x0123456789ABCDEF


def test_placed_statistics(engine):
    """over each plan kind: the sums over the first Le frames and count = min(Le, num_samples - first_frame) against the oracle, into
    records between canaries; with NULL spans the table of AADHip_WindowDecodePlanRunStats without rows"""
    import torch
    lib = engine.lib
    for kind, formats in (("plain", [(2, 3, True, MBS)] * 5), ("mixed", MIXED), ("mix1", CHANNEL), ("mix2", CHANNEL)):
        images, decoded, lengths, headers = _streams(formats, 14000)
        spbs = [h.num_samples_per_block for h in headers]
        frames = 2 * max(spbs) + 3
        windows, spans = _cases(lengths, spbs, frames)
        flat, table = _pack(images)
        d_img = torch.from_numpy(flat).cuda()
        channels = {"plain": 2, "mixed": 2, "mix1": 1, "mix2": 2}[kind]
        if kind == "plain":
            plan, rows16 = engine.window_decode_plan(headers[0], table, True), window_expected(decoded, windows, frames, 2)
        elif kind == "mixed":
            plan, rows16 = engine.mixed_window_decode_plan(headers, table, True), window_expected(decoded, windows, frames, 2)
        else:
            plan = engine.channel_mix_window_decode_plan(headers, table, channels, True)
            rows16 = channel_mix_expected(decoded, windows, frames, channels)
        try:
            n = len(windows)
            tables = Tables(torch, windows, spans, None)
            whole = torch.full((n * channels * 4 + 16,), REC_PATTERN, dtype=torch.int64, device="cuda")
            stats = whole[8:-8].view(n, channels, 4)
            assert plan.run(d_img, tables.windows, frames, stats=stats, rows=False, spans=tables.spans) is stats
            torch.cuda.synchronize()
            tables.assert_unchanged(kind)
            host = whole.cpu().numpy()
            assert (host[:8] == REC_PATTERN).all() and (host[-8:] == REC_PATTERN).all(), (kind, "wrote outside its records")
            want = po.placed_stats_expected(rows16, lengths, windows, spans)
            got = host[8:-8].reshape(n, channels, 4)
            assert np.array_equal(got, want), (kind, np.argwhere(got != want)[:3].tolist())
            assert (want[..., 0] > 0).sum() > n // 3 and (want[..., 3] == 0).sum() > 10 and (want[..., 3] < frames).any()
            # the engine's own helper takes the same road
            if kind == "plain":
                alone = plan.run(d_img, tables.windows, frames, stats=True, rows=False, spans=tables.spans)
                assert torch.equal(alone.cpu(), torch.from_numpy(want))
            # NULL spans: the statistics-only run without spans
            plain = plan.run(d_img, tables.windows, frames, stats=True, rows=False)
            whole.fill_(REC_PATTERN)
            torch.cuda.synchronize()  # a direct C call is not ordered against torch's stream
            assert lib.AADHip_WindowDecodePlanRunPlacedStats(plan.handle, d_img.data_ptr(), n, tables.windows.data_ptr(), None, frames,
                                                             stats.data_ptr()) == AADApiResult.OK
            torch.cuda.synchronize()
            assert torch.equal(stats, plain) and bool((plain[..., 3] > 0).any()), kind
        finally:
            plan.close()


# ---- 5. the event-mix recipe -----------------------------------------------------------------------------------------------------------
def test_mix_windows_with_noise_spans_is_its_two_runs(engine):
    import torch
    s_images, s_decoded = _channel_corpus()
    n_images, n_decoded = _mixed_corpus()

    def rows_of(images):
        data = torch.zeros((len(images), max(len(i) for i in images)), dtype=torch.uint8)
        for i, img in enumerate(images):
            data[i, :len(img)] = torch.frombuffer(bytearray(img), dtype=torch.uint8)
        return data

    s_data, n_data = rows_of(s_images), rows_of(n_images)
    s_sizes, n_sizes = [len(i) for i in s_images], [len(i) for i in n_images]
    n_lengths = [d.shape[0] for d in n_decoded]
    frames = 141
    s_windows = np.array([(s, f) for s in range(len(s_images)) for f in (0, 33, 200)] + [(len(s_images), 0)], dtype=np.int64)
    n_windows = np.array([((3 * k) % len(n_images), 17 * k) for k in range(len(s_windows))], dtype=np.int64)
    n_windows[3] = (len(n_images), 0)  # no noise there: gain 0
    spans = _i64([(20 + 9 * k, (37 * k) % 150) for k in range(len(s_windows))])
    spans[5] = (frames, 0)
    assert sum(le == 0 for le, _ in po.clipped(spans, len(spans), frames)) >= 1
    for channels in (1, 2):
        x32 = channel_mix_expected(s_decoded, s_windows, frames, channels, np.float32)
        y32 = channel_mix_expected(n_decoded, n_windows, frames, channels, np.float32)
        s_stats = channel_mix_stats_expected(s_decoded, s_windows, frames, channels)
        n_stats = po.placed_stats_expected(channel_mix_expected(n_decoded, n_windows, frames, channels), n_lengths, n_windows, spans)
        want_gains = snr_gains(torch.from_numpy(s_stats), torch.from_numpy(n_stats), 6.0)
        assert (want_gains > 0).sum() >= len(s_windows) - 8 and want_gains[3] == 0 and want_gains[-1] == 0
        unplaced = snr_gains(torch.from_numpy(s_stats), torch.from_numpy(channel_mix_stats_expected(n_decoded, n_windows, frames, channels)), 6.0)
        assert (unplaced != want_gains).sum() > len(s_windows) // 2  # the level of the event is not the level of the row
        for name in ("float32", "bfloat16"):
            rows, gains = engine.mix_windows((s_data.cuda(), s_sizes, torch.from_numpy(s_windows).cuda()),
                                             (n_data.cuda(), n_sizes, torch.from_numpy(n_windows).cuda()), frames, 6.0,
                                             dtype=go.torch_dtype(name), channels=channels, noise_spans=torch.from_numpy(spans).cuda())
            assert rows.dtype == go.torch_dtype(name) and rows.shape == (len(s_windows), channels, frames)
            assert torch.equal(gains.cpu(), want_gains), (channels, name)
            first = go.gain_expected(x32, np.ones(len(s_windows), dtype=np.float32), name)
            want = po.placed_expected(y32, spans, want_gains.numpy(), name, first)
            assert (want != first).any()
            _compare(go.bits_of(rows.cpu()), want, ("mix_windows", channels, name), s_windows)


# ---- 6. errors, through the C call -----------------------------------------------------------------------------------------------------
def test_argument_errors(engine):
    import torch
    lib, bad, ok = engine.lib, AADApiResult.INVALID_ARGUMENT, AADApiResult.OK
    frames = 100
    for label, plan, channels, flat, table, _ in _plans(engine):
        try:
            d_img = torch.from_numpy(flat).cuda()
            win = torch.tensor([[1, 0]], dtype=torch.int64, device="cuda")
            gain = torch.tensor([0.5, 0.25], dtype=torch.float32, device="cuda")
            span = torch.tensor([[7, 3], [9, 5]], dtype=torch.int64, device="cuda")
            out = torch.full((2 * channels * frames + 256,), CANARY, dtype=torch.int16, device="cuda")
            rec = torch.full((2 * channels * 4 + 16,), REC_PATTERN, dtype=torch.int64, device="cuda")
            run = lambda n, wp, sp, t, kind, op, gp, mode, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRunPlaced(
                plan.handle, data, n, wp, sp, t, kind, op, gp, mode)
            stat = lambda n, wp, sp, t, rp, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRunPlacedStats(
                plan.handle, data, n, wp, sp, t, rp)
            w, s, o, g = win.data_ptr(), span.data_ptr(), out.data_ptr(), gain.data_ptr()
            torch.cuda.synchronize()  # the direct C calls below are not ordered against torch's stream
            for kind in KINDS.values():
                for mode in (0, 1):
                    for off in (1, 2, 4):
                        assert run(1, w, s + off, frames, kind, o, g, mode) == bad, (label, "span table off 8-byte alignment", off)
                    assert run(1, w, s, frames, kind, o, g + 2, mode) == bad  # the gain run's refusals
                    assert run(1, w, s, frames, kind, None, g, mode) == bad
                    assert run(1, None, s, frames, kind, o, g, mode) == bad
                    assert run(1, w, s, frames, kind, o, g, mode, data=None) == bad
                    assert run(1, w, s, 0, kind, o, g, mode) == bad
                    assert run((1 << 63) // channels, w, s, 2, kind, o, g, mode) == bad
                    assert run(0, None, None, frames, kind, None, None, mode, data=None) == ok  # N = 0: nulls are fine
                    assert run(0, w, s, frames, kind, o, g, mode) == ok
                for mode in (2, -1, 1 << 8):
                    assert run(1, w, s, frames, kind, o, g, mode) == bad, (label, mode)
            for mode in (0, 1):
                assert run(1, w, s, frames, SAMPLE_INT16, o, g, mode) == bad  # int16 rows
                assert run(1, w, None, frames, SAMPLE_INT16, o, None, mode) == bad
                for kind in (2, 3, 6, -1):
                    assert run(1, w, s, frames, kind, o, g, mode) == bad
            r = rec.data_ptr() + 64
            for off in (1, 2, 4):
                assert stat(1, w, s + off, frames, r) == bad
            assert stat(1, w, s, frames, None) == bad and stat(1, w, s, frames, r + 4) == bad  # the statistics run's refusals
            assert stat(1, None, s, frames, r) == bad and stat(1, w, s, frames, r, data=None) == bad and stat(1, w, s, 0, r) == bad
            assert stat(0, None, None, frames, r, data=None) == ok
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == CANARY).all()  # no refused run and no N = 0 run wrote
            assert (rec.cpu().numpy() == REC_PATTERN).all()
            # a run on an `out` offset by 64 elements, a span table offset by one record: the canaries on both sides stay
            for kind, width in ((SAMPLE_FLOAT16, 1), (SAMPLE_FLOAT32, 2)):
                out.fill_(CANARY)
                torch.cuda.synchronize()
                assert run(1, w, s + 16, frames, kind, o + 64 * 2 * width, g + 4, 0) == ok
                torch.cuda.synchronize()
                host = out.cpu().numpy()
                lo, hi = 64 * width, 64 * width + channels * frames * width
                assert (host[:lo] == CANARY).all() and (host[hi:] == CANARY).all(), (label, kind)
                rows = host[lo:hi].reshape(channels, frames * width)
                assert (rows[:, :5 * width] == 0).all() and (rows[:, 14 * width:] == 0).all() and (rows[:, 5 * width:14 * width] != 0).any()
            assert stat(1, w, s + 16, frames, r) == ok
            torch.cuda.synchronize()
            host = rec.cpu().numpy()
            assert (host[:8] == REC_PATTERN).all() and (host[8 + 4 * channels:] == REC_PATTERN).all()
            assert (host[8:8 + 4 * channels].reshape(channels, 4)[:, 3] == 9).all()
        finally:
            plan.close()


# ---- 7. signal events ------------------------------------------------------------------------------------------------------------------
def test_signal_next_run_events_around_a_placed_run_of_several_kernels(engine):
    import torch
    from aad_amd.engine import HipEvent
    images, decoded = _mixed_corpus()
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)  # six variants: six kernels
    frames = 141
    windows_np = np.array([(s, (7 * s) % lengths[s]) for s in range(len(images))] * 8, dtype=np.int64)
    spans_np = _i64([(10 + 5 * k, 3 * k) for k in range(len(windows_np))])
    gain_np = np.linspace(-2, 2, len(windows_np)).astype(np.float32)
    windows, spans, gain = (torch.from_numpy(a).cuda() for a in (windows_np, spans_np, gain_np))
    side = torch.cuda.Stream()
    for add in (True, False):
        out = torch.full((len(windows_np), 2, frames), 0.25, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        start, stop = HipEvent(timing=True), HipEvent(timing=True)
        engine.signal_next(stop, start=start)
        plan.run(d_img, windows, frames, torch.float32, out=out, gain=gain, accumulate=add, ordered=False, spans=spans)
        stop.wait_on(side)
        with torch.cuda.stream(side):
            snapshot = out.clone()
        side.synchronize()
        old = np.full((len(windows_np), 2, frames), np.float32(0.25).view(np.uint32), dtype=np.uint32) if add else None
        want = po.placed_expected(window_expected(decoded, windows_np, frames, 2, np.float32), spans_np, gain_np, "float32", old)
        _compare(go.bits_of(snapshot.cpu()), want, ("events", add), windows_np)
        start.synchronize()
        stop.synchronize()
        assert start.elapsed_ms(stop) > 0
    # the statistics run: the start event in front of the clear, the stop event on the last kernel
    stats = torch.full((len(windows_np), 2, 4), REC_PATTERN, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    engine.signal_next(stop, start=start)
    plan.run(d_img, windows, frames, stats=stats, rows=False, ordered=False, spans=spans)
    stop.wait_on(side)
    with torch.cuda.stream(side):
        snapshot = stats.clone()
    side.synchronize()
    want = po.placed_stats_expected(window_expected(decoded, windows_np, frames, 2), lengths, windows_np, spans_np)
    assert torch.equal(snapshot.cpu(), torch.from_numpy(want))
    start.synchronize()
    stop.synchronize()
    assert start.elapsed_ms(stop) > 0
    plan.close()


# ---- 8. past the grid cap --------------------------------------------------------------------------------------------------------------
def test_store_on_float16_past_the_grid_cap(engine, policy, chip):
    """the geometry of tests/test_gpu_window_decode_gain.py::test_add_on_float16_past_the_grid_cap: 2^26 + 37 windows of two frames
    over stereo M/S 4-bit streams, 2^28 + 148 lanes under a grid capped at 2^20 workgroups - the last 37 windows are the second trip
    of the grid-stride loop.  A STORE run on float16 rows with spans of one frame or none, so that the lanes of a window's second
    block - and for an empty span both - have their fill and nothing else: the loop goes on past a lane that left early."""
    import torch
    ch, bits, frames, tail = 2, 4, 2, 37
    _, spb = spb_of(ch, bits, 64)
    first = 1 << 26
    n = first + tail
    plan = window_launch(policy, chip, n, frames, ch, bits, spb)
    assert plan.ok == 1 and plan.blocks_per_window == 2 and plan.workgroup == 256 and plan.grid == MAX_GRID and plan.lds == 0, plan
    assert plan.lanes == (1 << 28) + 4 * tail and plan.lanes % 64 != 0, plan
    need = n * 16 + n * 16 + n * 4 + n * ch * frames * 2 + (2 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("needs %.1f GiB of free device memory" % (need / 2 ** 30))
    images, decoded, lengths, headers = encoded_streams([(ch, bits, True, 64)] * 3, seed=6100)
    tile = window_tile(lengths, spb, frames, seed=61)
    last = np.array([(0, (1 + i % 3) * spb - 1) for i in range(tail)], dtype=np.int64)
    last[tail // 2] = (len(lengths), 0)
    kinds = [(1, 1), (1, 0), (0, 0), (2, 0), (5, 1), (1, 2)]
    tile_spans = _i64([kinds[i % len(kinds)] for i in range(P)])
    last_spans = _i64([kinds[(i + 1) % len(kinds)] for i in range(tail)])
    flat, table = pack_images(images)
    d_img = torch.from_numpy(flat).cuda()
    rng = np.random.default_rng(62)
    tile_gain, last_gain = rng.uniform(-2, 2, size=P).astype(np.float32), rng.uniform(-2, 2, size=tail).astype(np.float32)
    full = first // P

    def repeated(tile_np, last_np, dtype, width):
        t = torch.empty((n, width) if width else (n,), dtype=dtype, device="cuda")
        tile_d = torch.from_numpy(tile_np).cuda()
        t[:full * P].view((full, P, width) if width else (full, P)).copy_(tile_d.unsqueeze(0).expand((full,) + tuple(tile_d.shape)))
        t[full * P:first] = tile_d[:first - full * P]
        t[first:] = torch.from_numpy(last_np).cuda()
        return t

    windows = repeated(tile, last, torch.int64, 2)
    spans = repeated(tile_spans, last_spans, torch.int64, 2)
    gains = repeated(tile_gain, last_gain, torch.float32, 0)
    whole = torch.full((n * ch * frames + 2 * GUARD,), CANARY, dtype=torch.int16, device="cuda")
    y = whole[GUARD:-GUARD].view(torch.float16).view(n, ch, frames)
    p = engine.window_decode_plan(headers[0], table, True)
    try:
        p.run(d_img, windows, frames, torch.float16, out=y, gain=gains, spans=spans)
        torch.cuda.synchronize()
    finally:
        p.close()
    assert bool((whole[:GUARD] == CANARY).all()) and bool((whole[-GUARD:] == CANARY).all()), "wrote outside its rows"
    exp = po.placed_expected(window_expected(decoded, tile, frames, ch, np.float32), tile_spans, tile_gain, "float16")
    exp_last = po.placed_expected(window_expected(decoded, last, frames, ch, np.float32), last_spans, last_gain, "float16")
    assert (exp != 0).any() and (exp_last != 0).any() and (exp_last == 0).any()
    got, got_last = go.bits_of(y[:P].cpu()), go.bits_of(y[first:].cpu())
    assert np.array_equal(got, exp), ("first tile", np.argwhere(got != exp)[:3].tolist())
    assert np.array_equal(got_last, exp_last), ("the second trip's windows", np.argwhere(got_last != exp_last)[:3].tolist())
    reps = y[:full * P].view(torch.int16).view(full, P * ch * frames)
    assert bool((reps == reps[0]).all()), "a repetition of the tile differs"
    del windows, spans, gains, whole, y, reps
    torch.cuda.empty_cache()
