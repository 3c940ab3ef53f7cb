"""tests/resample_rows_oracle.py, with no GPU: the chunked FIR on given rows against tests/resample_oracle.py's definition, its
wrappers against the originals, and the conditions on the case tables of tests/test_gpu_resample_geometry.py -
  * every bank of the plain and the three wide sets, shifts below, at and above the lead, rows shorter than the reach, chunks of
    one output and of all;
  * full tiles: at T = 4097 every ratio outside the exempt list has a full tile n0 > 0 that spans floor(1023 M / L) + 1 source
    frames, and the exempt ones provably have none at any n0;
  * the 2^31 shapes: (T - 1) M < 2^31 <= T M for the bank that sets the limit, and T_src as the issue states it;
  * the item loop: every ordered triple of kinds at least 8 times among the workgroups that take three items;
  * past 4 GiB: a row straddles each named boundary of each buffer, 16 witness rows on both sides and at both ends, rows that
    alternate 4-byte alignment, at least 64 rows wholly above element 2^32 and more than 2^22 items."""
import itertools

import numpy as np
import pytest

import resample_mix_oracle as mo
import resample_oracle as ro
import resample_rows_oracle as rr

ALL_RATIOS = sorted({r for ratios, _ in rr.resamplers().values() for r in ratios} | set(rr.BIG_WIDE) |
                    {r for s in rr.LIMIT_SHAPES.values() for r in s["ratios"]})
_BANKS = {}


def _bank(L, M):
    if (L, M) not in _BANKS:
        _BANKS[L, M] = ro.bank(L, M)
    return _BANKS[L, M]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", ALL_RATIOS, ids=["%d_%d" % r for r in ALL_RATIOS])
def test_fir_rows_equals_the_definition(ratio):
    L, M = ratio
    h = _bank(L, M)
    K = h.shape[1]
    lead = K // 2 - 1
    rng = np.random.default_rng(L * 65537 + M)
    frames = 70
    needed = (frames - 1) * M // L + K
    for t_src in (needed, needed + 1, max(needed // 2, 1), max(lead, 1), 1):  # whole, and shorter than the reach
        x = rng.integers(-32768, 32768, size=t_src).astype(np.int16)
        x[::5] = rng.choice([-32768, 32767], size=len(x[::5]))
        for shift in sorted({0, 1, max(lead - 1, 0), lead, lead + 3, t_src - 1, t_src, t_src + K}):
            want = ro.fir(x, shift, frames, L, M, h)
            assert np.array_equal(rr.fir_rows(x, shift, frames, L, M, h), want), (t_src, shift)
            assert np.array_equal(rr.fir_many(x[None], [shift], frames, L, M, h, budget=1)[0], want), (t_src, shift, "one output a chunk")
    assert np.abs(want).max() == 0 and np.abs(ro.fir(x, 0, frames, L, M, h)).max() > 0


def test_fir_many_takes_a_row_and_a_shift_each():
    L, M = 160, 441
    h = _bank(L, M)
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, size=(7, 900)).astype(np.int16)
    shifts = [0, 1, 33, 36, 500, 899, 2000]
    for budget in (1 << 22, 5000):
        got = rr.fir_many(x, shifts, 300, L, M, h, budget=budget)
        for r in range(7):
            assert np.array_equal(got[r], ro.fir(x[r], shifts[r], 300, L, M, h)), (budget, r)


def test_wrappers_equal_the_originals():
    banks = [(L, M, _bank(L, M)) for L, M in ((1, 1), (10, 9), (1, 3))]
    rng = np.random.default_rng(11)
    frames, channels = 50, 2
    t_src = ro.source_frames(frames, [(L, M, h.shape[1]) for L, M, h in banks])
    lanes = np.array([(0, 0), (1, 11), (2, 40), (ro.NO_BANK, 3), (1, 0), (7, 2)], dtype=np.int64)
    src = rng.integers(-32768, 32768, size=(len(lanes) * channels, t_src)).astype(np.int16)
    acc = rr.expected_acc(src, lanes, banks, frames, channels)
    for w, (b, shift) in enumerate(lanes.tolist()):
        for c in range(channels):
            want = ro.fir(src[w * channels + c], shift, frames, *banks[b]) if b < len(banks) else np.zeros(frames, dtype=np.int64)
            assert np.array_equal(acc[w, c], want), (w, c)
    spans = rr.spans_for(len(lanes), frames)
    c_src = np.array([0, 5, 12, 40, t_src, t_src + 9, 3, 3, 1, 200, 7, 7], dtype=np.int64)
    for sp in (None, spans):
        counts = rr.output_counts(c_src, t_src, lanes, banks, frames, sp, channels)
        for w, (b, shift) in enumerate(lanes.tolist()):
            for c in range(channels):
                le = rr.po.clipped(sp, len(lanes), frames)[w][0]
                want = mo.output_count_brute(c_src[w * channels + c], t_src, shift, banks[b][0], banks[b][1], le) if b < len(banks) else 0
                assert counts[w, c] == want, (w, c)
        same = np.repeat(counts[:, :1], channels, axis=1)  # one count per window: the original's shape
        assert np.array_equal(rr.stats_of(acc, sp, same), mo.expected_stats(acc, sp, same[:, 0]))
        assert np.array_equal(rr.stats_of(acc, sp, counts)[..., :3], mo.expected_stats(acc, sp, same[:, 0])[..., :3])
        assert np.array_equal(rr.stats_of(acc, sp, counts)[..., 3], counts)
    assert (counts > 0).any() and (counts == 0).any()


def test_kernel_list():
    assert len(rr.KERNELS) == 15 and len(set(rr.KERNELS)) == 15 and len({rr.run_id(r) for r in rr.RUNS}) == 16
    acc = np.arange(-12, 12, dtype=np.int64).reshape(2, 1, 12) << 22
    gains = np.array([0.5, -3.0], dtype=np.float32)
    spans = np.array([(5, 2), (12, 0)], dtype=np.int64)
    old = ro.convert(acc[::-1], "float32")
    zero = np.zeros((2, 1), dtype=np.int64)
    rows, rec = rr.kernel_expected(("rows", "int16", False), acc, spans, gains, old, zero, zero)
    assert rec is None and np.array_equal(rows, ro.convert(acc, "int16"))
    rows, _ = rr.kernel_expected(("gain", "float32", True), acc, spans, gains, old, zero, zero)
    assert np.array_equal(rows, mo.expected_rows(acc, spans, gains, "float32", old))
    rows, _ = rr.kernel_expected(("gain", "float32", False), acc, spans, gains, old, zero, zero)
    assert np.array_equal(rows, mo.expected_rows(acc, spans, gains, "float32"))
    rows, rec = rr.kernel_expected(("stats", None, True), acc, spans, gains, old, zero + 1, zero + 2)
    assert rows is None and (rec[..., 3] == 2).all() and rec[0, 0, 1] == np.abs(ro.convert(acc[0, 0, :5], "int16").astype(np.int64)).sum()


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
def test_ratio_sets():
    for name, (ratios, wide) in rr.resamplers().items():
        assert len(set(ratios)) == len(ratios) and (1, 1) in ratios
        assert all(ro.reduce_ratio(*r) == r for r in ratios)
        if wide:
            assert ratios[:len(rr.WIDE_SETS[name])] == rr.WIDE_SETS[name] and rr.gather_round(ratios) == rr.ROUNDS[name]
            assert sum(1 for r in ratios if rr.gathered(*r)) >= 2 and sum(1 for r in ratios if not rr.gathered(*r)) >= 3
        else:
            assert all(ro.limits_ok(*r) for r in ratios)
    assert sorted(rr.ROUNDS.values()) == [64, 128, 256]
    assert 2 * 1024 * ro.taps(1024, 1365) == 65536 and ro.taps(3, 32) == 256 and ro.limits_ok(3, 32)  # the resident limit; the most taps


# ---- a. full tiles -------------------------------------------------------------------------------------------------------------------
def test_every_ratio_has_a_full_tile_with_the_extra_frame_or_is_exempt():
    T = rr.FULL_TILE_FRAMES
    assert T == 4097 and (T - 1) // rr.TILE == 4
    seen = set()
    for ratios, _ in rr.resamplers().values():
        for L, M in ratios:
            seen.add((L, M))
            tiles = rr.extra_frame_tiles(L, M, T)
            if (L, M) in rr.EXEMPT:
                assert (1024 * M) % L == 0 or (1023 * M) % L == 0  # whole frames per tile, or per 1023 outputs
                assert not rr.extra_frame_tiles(L, M, 64 * rr.TILE + 1)  # at no tile at all
            else:
                assert tiles and min(tiles) <= 3 * rr.TILE, (L, M)
                assert all(0 < n0 and n0 + rr.TILE <= T - 1 for n0 in tiles)
    assert set(rr.EXEMPT) <= seen


def test_span_sets_put_a_bank_with_a_last_tap_in_charge_of_the_span():
    T = rr.FULL_TILE_FRAMES
    for name, (ratios, wide) in rr.SPAN_SETS.items():
        banks = [(L, M, _bank(L, M)) for L, M in ratios]
        L, M, h = banks[0]
        K = h.shape[1]
        assert (L, M) not in rr.EXEMPT and rr.gathered(L, M) == wide
        assert rr.span_elements(L, M, K) == max(rr.span_elements(l, m, g.shape[1]) for l, m, g in banks)
        ends = [h[(n0 + rr.TILE - 1) * M % L][K - 2:] for n0 in rr.extra_frame_tiles(L, M, T)]
        assert ends and any(e.any() for e in ends)
        t_src = ro.source_frames(T, [(l, m, g.shape[1]) for l, m, g in banks])
        lanes, _ = rr.full_tile_lanes(banks, t_src, T)
        src = np.random.default_rng(5).integers(-32768, 32768, size=(len(lanes) * 2, t_src)).astype(np.int16)
        found = rr.short_span_witnesses(src, lanes, banks, t_src, T, 2)
        assert found and all(lanes[row // 2, 0] == 0 for row, _, _ in found)
        row, n, delta = found[0]
        shift = int(lanes[row // 2, 1])
        acc = rr.fir_rows(src[row], shift, T, L, M, h)
        cut = src[row].copy()
        j = shift + n * M // L + K - 1 - (K // 2 - 1)
        cut[j - 1:j + 1] = 0  # the two frames under the last two taps of output n - and under earlier taps of no output before it
        assert acc[n] - rr.fir_rows(cut, shift, T, L, M, h)[n] == delta
    # every set above: the widest bank's phases end in zeros, at the last output of every full tile
    for ratios, _ in rr.resamplers().values():
        L, M = max(ratios, key=lambda r: rr.span_elements(r[0], r[1], ro.taps(*r)))
        h = _bank(L, M)
        assert not any(h[(n0 + rr.TILE - 1) * M % L][-2:].any() for n0 in (1024, 2048, 3072)), (L, M)


def test_full_tile_lanes():
    T = rr.FULL_TILE_FRAMES
    banks = [(L, M, np.zeros((1, ro.taps(L, M)), dtype=np.int16)) for L, M in rr.PLAIN]
    t_src = ro.source_frames(T, [(L, M, h.shape[1]) for L, M, h in banks])
    lanes, counts = rr.full_tile_lanes(banks, t_src, T)
    assert len(lanes) == 5 * len(banks)
    for b, (L, M, h) in enumerate(banks):
        lead = h.shape[1] // 2 - 1
        mine = lanes[lanes[:, 0] == b]
        assert mine[:4, 1].tolist() == [0, 1, lead, lead + 3]
        late = int(mine[4, 1])
        n_first_zero = [n for n in range(T) if late + n * M // L >= t_src][0]  # the centre tap leaves the row
        assert 2 * rr.TILE < n_first_zero < 3 * rr.TILE
    assert (counts == 0).any() and (counts == t_src).any() and (counts > t_src).any() and ((counts > 0) & (counts < t_src)).any()
    spans = rr.spans_for(11, T).tolist()
    o, le = spans[1][1], spans[1][0]
    assert o % 2 == 1 and o < 1024 and o + le > 3072  # across 1024, 2048 and 3072 from an odd offset
    assert [7, 8] == [spans[7][1], spans[8][1]]


# ---- d. the 2^31 limit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.LIMIT_SHAPES))
def test_limit_shapes(name):
    s = rr.LIMIT_SHAPES[name]
    T = s["frames"]
    M = max(M for _, M in s["ratios"])
    assert (T - 1) * M < 1 << 31 <= T * M
    assert all((T - 1) * m < 1 << 31 for _, m in s["ratios"])
    assert ro.source_frames(T, [(L, m, ro.taps(L, m)) for L, m in s["ratios"]]) == s["source_frames"]
    assert all(ro.limits_ok(*r) for r in s["ratios"]) != s["wide"]
    if s["wide"]:
        assert (T - 1) * 10933 == 2147481726 and ro.taps(1025, 10933) == 256 and T % rr.TILE not in (0, 1)  # the last tile is partial
        assert (T % rr.TILE) % 64 != 0  # and so is its last round
    assert T // rr.TILE > 100  # n0 in the hundreds of tiles


# ---- c. the item loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.resamplers()))
def test_item_triples(name):
    ratios, wide = rr.resamplers()[name]
    kinds, identity = rr.item_kinds(ratios, wide)
    assert ratios[identity] == (1, 1) and kinds[0] is None and identity not in kinds
    assert len(set(kinds)) == len(kinds) == (5 if wide else 4)
    if wide:
        flags = [rr.gathered(*ratios[k]) for k in kinds[1:]]
        assert flags == [False, False, True, True]
        assert max(ro.taps(*ratios[k]) for k in kinds[3:]) == max(ro.taps(*r) for r in ratios if rr.gathered(*r))
    triples = rr.item_triples(kinds)
    assert triples.shape == (rr.ITEM_EXTRA, 3) and rr.ITEM_EXTRA % 1024 == 0
    count = {t: 0 for t in itertools.product(range(len(kinds)), repeat=3)}
    for t in triples.tolist():
        count[tuple(t)] += 1
    assert len(count) == len(kinds) ** 3 and min(count.values()) >= 8
    assert rr.item_rows() == 2 * rr.GRID + rr.ITEM_EXTRA and rr.item_rows() * ((rr.ITEM_FRAMES - 1) // rr.TILE + 1) > 2 * rr.GRID


# ---- e. past 4 GiB -------------------------------------------------------------------------------------------------------------------
def test_big_placements():
    T, rows = rr.BIG_FRAMES, 2 * rr.BIG_WINDOWS
    t_src = rr.big_source_frames()
    assert T % 2 == 1 and t_src % 2 == 1  # rows alternate 4-byte alignment in the int16 buffers
    assert rows * T > 1 << 32 and rows - -(-(1 << 32) // T) >= 64  # rows wholly above element 2^32
    assert rows * ((T - 1) // rr.TILE + 1) > 1 << 22 and (T - 1) // rr.TILE + 1 == 5
    witnesses = set(rr.big_witness_windows().tolist())
    assert len(witnesses) < 400
    for name, (pitch, size, elements) in rr.big_boundaries().items():
        want = {"int16": 2, "float32": 3, "source": 2}[name]
        assert len(set(elements)) == want
        assert {e * size for e in elements} >= {1 << b for b in ((32, 33, 34) if name == "float32" else (32, 33))}
        assert {1 << 31, 1 << 32} <= set(elements)
        for e in elements:
            r = e // pitch
            assert e % pitch != 0 and r * pitch < e < (r + 1) * pitch <= rows * pitch, (name, e)  # row r straddles it
            assert r + 16 < rows
            assert {q // 2 for q in range(r - 16, r + 17)} <= witnesses
    assert set(range(8)) <= witnesses and set(range(rows // 2 - 8, rows // 2)) <= witnesses
    assert max(witnesses) == rows // 2 - 1
    for ratios in (rr.BIG_PLAIN, rr.BIG_WIDE):
        assert ro.source_frames(T, [(L, M, ro.taps(L, M)) for L, M in ratios]) == t_src - 1 and t_src < T + 400
    assert [rr.gathered(*r) for r in rr.BIG_WIDE] == [False, False, False, True]


# ---- the vectorised rows and records ---------------------------------------------------------------------------------------------------
def test_run_expected_equals_the_originals():
    import torch
    rng = np.random.default_rng(23)
    n, channels, frames = 14, 2, 40
    acc = rng.integers(-(1 << 30), 1 << 30, size=(n, channels, frames))
    acc[3] = 0  # a window without a bank
    acc[5, 1, :7] = [(1 << 31) - 1, -(1 << 31) + 1, 8191, 8192, -8193, 16384 * 32767 + 8192, -16384 * 32768 - 9000]
    spans = rr.spans_for(n, frames)
    gains = rng.uniform(-2, 2, size=n).astype(np.float32)
    gains[:4] = [1.0, -1.0, 0.0, -0.5]
    le, o = rr.clipped_rows(spans, n, frames, channels)
    hard = np.array([(-1, 3), (10, 1 << 40), (10, -5), (1 << 62, frames - 1), (0, 0), (3, frames), (frames + 5, 0)], dtype=np.int64)
    for sp in (spans, hard):
        pairs = rr.po.clipped(sp, len(sp), frames)
        got = rr.clipped_rows(sp, len(sp), frames, 1)
        assert [p[0] for p in pairs] == got[0].tolist() and [p[1] for p in pairs] == got[1].tolist()
    assert (le == 0).any() and (o % 2 == 1).any() and (le == frames).any()
    rows = n * channels
    counts_full = rng.integers(0, frames + 1, size=(n, channels))
    counts_span = np.minimum(counts_full, le.reshape(n, channels))
    e = torch.arange(rows * frames, dtype=torch.int64).reshape(rows, frames) + (1 << 33)
    for run in rr.RUNS:
        kind, name, flag = run
        old = rr.old_pattern(e, name) if kind == "gain" else None
        old_bits = None if old is None else rr.bit_view(old).numpy().view(np.uint32 if name == "float32" else np.uint16).reshape(acc.shape)
        want_rows, want_rec = rr.kernel_expected(run, acc, spans, gains, old_bits, counts_full, counts_span)
        got_rows, got_rec = rr.run_expected(run, acc.reshape(rows, frames), le, o, np.repeat(gains, channels), old,
                                            counts_full.reshape(-1), counts_span.reshape(-1))
        assert (want_rows is None) == (got_rows is None) and (want_rec is None) == (got_rec is None), run
        if want_rows is not None:
            got = rr.bit_view(got_rows).numpy().reshape(acc.shape)
            assert np.array_equal(got.view(want_rows.dtype), want_rows), run
        if want_rec is not None:
            assert np.array_equal(got_rec.numpy().reshape(n, channels, 4), want_rec), run
    old = rr.old_pattern(torch.arange(1000, dtype=torch.int64), "bfloat16")
    assert old.float().abs().max() < 1 and torch.equal(old.float(), rr.old_pattern(torch.arange(1000, dtype=torch.int64), "float32"))
    c = rr.identity_counts(torch.tensor([0, 3, 9, 50, 50]), 20, torch.tensor([2, 3, 2, 1, 0]), torch.tensor([9, 9, 5, 9, 30]))
    assert c.tolist() == [mo.output_count(cs, 20, s, 1, 1, le_) for cs, s, le_ in ((0, 2, 9), (3, 3, 9), (9, 2, 5), (50, 1, 9), (50, 0, 30))]
