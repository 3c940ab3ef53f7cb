"""The resample stage's C calls on hand-made source rows (AADHip_ResamplerRun, ...RunGain, ...RunStats; include/aad_hip.h
"resample") for LARGE shapes, and the case tables of tests/test_gpu_resample_geometry.py as pure functions, so that
tests/test_resample_geometry_host.py can hold both with no GPU:

  fir_rows / fir_many   acc of rows whose source row is given directly - element j of the row, zero for j < 0 and j >= T_src - by
                        the header's rule j = shift + i + k - (K/2 - 1), in chunks of outputs; held equal to resample_oracle.fir;
  kernel_expected       what each of the 15 FIR kernels of a resampler writes for given acc, spans, gains, old rows and source
                        counts, through resample_oracle.convert and resample_mix_oracle.expected_rows / expected_stats / output_count;
  the tables            ratio sets, the full-tile condition, the 2^31 shapes, the item-loop triples, the 4 GiB placements.

TEST INFRASTRUCTURE (tests/ only)."""
import itertools

import numpy as np

import resample_mix_oracle as mo
import resample_oracle as ro
import window_placed_oracle as po

TILE = 1024          # outputs of one workgroup's tile (aad_resample.h kResampleTile)
GRID = 1 << 20       # workgroups of the largest grid (resample_grid): the item loop takes the rest
DTYPES = ("int16", "float32", "float16", "bfloat16")
FLOATS = ("float32", "float16", "bfloat16")

# ---- ratio sets ----------------------------------------------------------------------------------------------------------------------
RESIDENT = [(1, 1), (10, 9), (160, 441)]
# a plain resampler: the resident ratios, those of the rails test, a bank of exactly 65536 bytes and one with K = 256
PLAIN = RESIDENT + [(3, 1), (1, 3), (147, 160), (1024, 1365), (3, 32)]
# tests/test_gpu_resample_wide.SETS (asserted equal on the GPU side): rounds of 64, 128 and 256
WIDE_SETS = {"all": [(1600, 3969), (1600, 4851), (1600, 1617), (1025, 1), (1024, 1367), (1025, 10933), (4099, 4098)] + RESIDENT,
             "round256": [(1600, 3969), (1600, 4851), (4099, 4098), (1, 1)],
             "round128": [(331, 1370), (1600, 3969), (10, 9)]}
ROUNDS = {"all": 64, "round256": 256, "round128": 128}
# L divides 1024 M (every tile starts on a whole source frame) or 1023 M (a tile's 1023 steps are whole frames): no tile n0 = 1024 t
# spans floor(1023 M / L) + 1 source frames
EXEMPT = [(1, 1), (3, 1), (1, 3), (3, 32), (1024, 1365), (1024, 1367)]


# The span of a tile in LDS is sized for the resampler's widest bank, and that bank's last taps are zeros in every set above (a
# Kaiser window's edge, floored): a span that is short for it changes no value.  These two put a bank whose phases end in a
# non-zero tap in charge of the span, so that the last output of a full tile reads a coefficient that counts from the span's end.
SPAN_SETS = {"span-plain": ([(10, 9)], False), "span-wide": ([(1600, 1617), (1, 1)], True)}  # the identity's span is 1030 elements


def short_span_witnesses(src, lanes, banks, t_src, frames, channels, pointer_parity=0):
    """rows [N * C, T_src], lanes [N, 2] -> [(row, n, delta)]: outputs n = n0 + 1023 of a full tile n0 > 0 that spans
    floor(1023 M / L) + 1 source frames, in a row whose span starts one element in front (`front` = 1: the span is at its
    longest), with delta != 0 the part of acc[n] that the last two taps carry - what a span one word shorter than the tile needs
    would lose"""
    out = []
    for row in range(len(lanes) * channels):
        bank, shift = (int(v) for v in lanes[row // channels])
        if bank >= len(banks):
            continue
        L, M, h = banks[bank]
        K = h.shape[1]
        for n0 in extra_frame_tiles(L, M, frames):
            front = (pointer_parity + row * t_src + shift + n0 * M // L - (K // 2 - 1)) & 1
            n = n0 + TILE - 1
            j = shift + n * M // L + K - 1 - (K // 2 - 1)  # the last tap's frame
            if front == 1 and j < t_src:
                delta = int(h[n * M % L][K - 1]) * int(src[row, j]) + int(h[n * M % L][K - 2]) * int(src[row, j - 1])
                if delta != 0:
                    out.append((row, n, delta))
    return out


def gathered(L, M):
    return not ro.limits_ok(L, M)


def wide_ratios(name):
    """the set `name` with the resident ratios it lacks behind it: the identity carries the bulk rows of the large cases, and the
    item loop wants two resident banks; a resident bank does not change the round (that of the gathered bank with the most taps)"""
    return WIDE_SETS[name] + [r for r in RESIDENT if r not in WIDE_SETS[name]]


def resamplers():
    """name -> (ratios, wide)"""
    out = {"plain": (PLAIN, False)}
    out.update({name: (wide_ratios(name), True) for name in WIDE_SETS})
    return out


def span_elements(L, M, K):
    """aad_resample.h resample_span_elements"""
    return ((TILE - 1) * M // L + 1 + K + 1 + 2 + 1) // 2 * 2


def gather_round(ratios):
    """R of a wide resampler (aad_resample.h resample_gather_round of the gathered bank with the most taps), 0 without one"""
    ks = [ro.taps(L, M) for L, M in ratios if gathered(L, M)]
    if not ks:
        return 0
    K = max(ks)
    stride = K + 2 if (K // 2) % 2 == 0 else K
    R = 256
    while R > 64 and R * (2 * stride + 4) > 40960:
        R //= 2
    return R


# ---- the FIR on given rows -------------------------------------------------------------------------------------------------------------
def fir_many(x, shifts, frames, L, M, h, budget=1 << 22):
    """x: int array [R, T_src], one source row each; shifts: [R] -> int64 acc [R, frames] with bank (L, M, h[L, K]).
    A chunk of outputs is gathered into [R, n, K] and reduced in float64: every product is below 2^31 and every partial sum of a
    phase below 32768 * 65535 < 2^31 (sum |h| <= 65535), far below 2^53, so float64 is exact here."""
    h = np.asarray(h)
    K = h.shape[1]
    x = np.asarray(x)
    R, t_src = x.shape
    shifts = np.asarray(shifts, dtype=np.int64).reshape(R)
    lead = K // 2 - 1
    xp = np.zeros((R, lead + t_src + 1), dtype=np.float64)  # column j + lead holds element j; the last one is the zero past the row
    xp[:, lead:lead + t_src] = x
    hf = h.astype(np.float64)
    out = np.zeros((R, frames), dtype=np.int64)
    step = max(budget // (K * R), 1)
    k = np.arange(K, dtype=np.int64)
    rows = np.arange(R)[:, None, None]
    for a in range(0, frames, step):
        n = np.arange(a, min(a + step, frames), dtype=np.int64)
        i, p = n * M // L, n * M % L
        at = shifts[:, None, None] + i[None, :, None] + k[None, None, :]  # j + lead >= 0
        np.minimum(at, xp.shape[1] - 1, out=at)  # the last column is a zero
        out[:, a:a + len(n)] = np.rint(np.einsum("rnk,nk->rn", xp[rows, at], hf[p])).astype(np.int64)
    assert np.abs(out).max(initial=0) < 1 << 31
    return out


def fir_rows(x, shift, frames, L, M, h):
    """one source row x[T_src] and its lane's shift -> int64 acc[frames]"""
    return fir_many(np.asarray(x)[None, :], [shift], frames, L, M, h)[0]


def expected_acc(src, lanes, banks, frames, channels):
    """src: int16 [N * C, T_src]; lanes: [N, 2] of (bank, shift), bank >= len(banks): none -> int64 acc [N, C, frames]"""
    lanes = np.asarray(lanes, dtype=np.int64).reshape(-1, 2)
    n = len(lanes)
    assert src.shape[0] == n * channels
    acc = np.zeros((n * channels, frames), dtype=np.int64)
    row_bank = np.repeat(lanes[:, 0], channels)
    row_shift = np.repeat(lanes[:, 1], channels)
    for b, (L, M, h) in enumerate(banks):
        rows = np.nonzero(row_bank == b)[0]
        for a in range(0, len(rows), 64):
            part = rows[a:a + 64]
            acc[part] = fir_many(src[part], row_shift[part], frames, L, M, h)
    return acc.reshape(n, channels, frames)


def output_counts(c_src, t_src, lanes, banks, frames, spans, channels):
    """mo.output_count per row: c_src [N * C] crafted source counts -> int64 [N, C]"""
    lanes = np.asarray(lanes, dtype=np.int64).reshape(-1, 2)
    les = po.clipped(spans, len(lanes), frames)
    out = np.zeros((len(lanes), channels), dtype=np.int64)
    for w, (bank, shift) in enumerate(lanes.tolist()):
        if bank < len(banks):
            L, M, _ = banks[bank]
            for c in range(channels):
                out[w, c] = mo.output_count(int(c_src[w * channels + c]), t_src, shift, L, M, les[w][0])
    return out


def stats_of(acc, spans, counts):
    """mo.expected_stats with a count per ROW (the source counts are crafted per row): acc [N, C, T]; counts [N, C]"""
    out = mo.expected_stats(acc, spans, np.zeros(acc.shape[0], dtype=np.int64))
    out[..., 3] = counts
    return out


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------
# (kind, sample type or None, flag): the 15 FIR kernels a resampler launches; flag: gain - ADD; stats - with spans (no rows alone)
KERNELS = ([("rows", t, False) for t in DTYPES] + [("gain", t, add) for t in FLOATS for add in (False, True)] +
           [("stats", t, False) for t in DTYPES] + [("stats", None, False)])
RUNS = KERNELS + [("stats", None, True)]  # the statistics-only kernel once more, over spans


def run_id(run):
    kind, name, flag = run
    if kind == "gain":
        return "gain-%s-%s" % (name, "add" if flag else "store")
    if kind == "stats":
        return "stats-%s%s" % (name or "norows", "-spans" if flag else "")
    return "rows-%s" % name


def kernel_expected(run, acc, spans, gains, old_bits, counts_full, counts_span):
    """-> (rows' bit patterns or None, int64 records or None) of one run over acc [N, C, T]; the gain runs and the statistics
    over spans take `spans`, every other run the whole row"""
    kind, name, flag = run
    if kind == "rows":
        return ro.convert(acc, name), None
    if kind == "gain":
        return mo.expected_rows(acc, spans, gains, name, old_bits if flag else None), None
    if flag:
        return None, stats_of(acc, spans, counts_span)
    return (None if name is None else ro.convert(acc, name)), stats_of(acc, None, counts_full)


# ---- a. full tiles behind the first ------------------------------------------------------------------------------------------------------
FULL_TILE_FRAMES = 4 * TILE + 1


def extra_frame_tiles(L, M, frames):
    """the tiles n0 > 0, full, of a row of `frames` outputs that span floor(1023 M / L) + 1 source frames"""
    return [n0 for n0 in range(TILE, frames - TILE + 1, TILE)
            if (n0 + TILE - 1) * M // L - n0 * M // L == (TILE - 1) * M // L + 1]


def full_tile_lanes(banks, t_src, frames):
    """five windows per bank: shifts 0, 1, lead, lead + 3, and one whose last source frame lies under the taps of output 2600 -
    the third tile ends in zeros; with crafted source counts 0, below shift, mid-row, T_src -> (lanes [N, 2], c_src per window)"""
    lanes, counts = [], []
    for b, (L, M, h) in enumerate(banks):
        lead = h.shape[1] // 2 - 1
        late = t_src - 2600 * M // L
        assert late > lead and 2600 < frames
        for k, shift in enumerate((0, 1, lead, lead + 3, late)):
            lanes.append((b, shift))
            counts.append((0, max(shift - 1, 0), shift + (frames // 2) * M // L, t_src, t_src + 5)[(k + b) % 5])
    return np.array(lanes, dtype=np.int64), np.array(counts, dtype=np.int64)


def spans_for(n, frames):
    """spans in output frames: whole, across elements 1024, 2048 and 3072 where the row has them, odd and even offsets, clipped, empty"""
    T = frames
    kinds = [(T, 0), (T - T // 4, T // 5 - (T // 5) % 2 + 1), (0, 0), (5, 0), (T, 1), (10, T - 1), (10, T), (T // 2, 7), (T // 2, 8),
             (T - 9, 9), (-1, 3)]
    return np.array(kinds, dtype=np.int64)[np.arange(n) % len(kinds)]


# ---- d. the 2^31 limit -----------------------------------------------------------------------------------------------------------------
LIMIT_SHAPES = {"wide": dict(ratios=[(1025, 10933), (160, 441), (1, 1)], wide=True, frames=196423, source_frames=2095360),
                "plain": dict(ratios=[(1024, 1365), (147, 160), (1, 1)], wide=False, frames=1573249, source_frames=2097183)}


# ---- c. the item loop ------------------------------------------------------------------------------------------------------------------
ITEM_FRAMES = 9
ITEM_EXTRA = 1024  # E: the workgroups that take a third item


def item_kinds(ratios, wide):
    """the kinds a designed row takes, as bank indices (None: no bank), and the identity bank of the bulk"""
    identity = ratios.index((1, 1))
    if not wide:
        return [None] + [ratios.index(r) for r in ((1024, 1365), (3, 32), (147, 160))], identity
    res = [ratios.index(r) for r in ratios if not gathered(*r) and r != (1, 1)][:2]
    g = [r for r in ratios if gathered(*r)]
    most = max(g, key=lambda r: ro.taps(*r))
    other = [r for r in g if r != most][0]
    return [None] + res + [ratios.index(other), ratios.index(most)], identity


def item_triples(kinds, extra=ITEM_EXTRA):
    """[extra, 3]: the kinds of rows b, 2^20 + b and 2^21 + b of workgroup b < extra - every ordered triple in turn"""
    triples = list(itertools.product(range(len(kinds)), repeat=3))
    return np.array([triples[b % len(triples)] for b in range(extra)], dtype=np.int64)


def item_rows(extra=ITEM_EXTRA):
    return 2 * GRID + extra


# ---- e. past 4 GiB ---------------------------------------------------------------------------------------------------------------------
BIG_FRAMES = 4099
BIG_WINDOWS = 524200  # C = 2: 1 048 400 rows
BIG_PLAIN = [(1, 1), (10, 9), (147, 160)]
BIG_WIDE = BIG_PLAIN + [(4099, 4098)]


def big_source_frames():
    """T_src of both resamplers (147/160 sets it) and one more: an odd pitch, so the source rows alternate 4-byte alignment too"""
    needed = ro.source_frames(BIG_FRAMES, [(L, M, ro.taps(L, M)) for L, M in BIG_WIDE])
    assert needed % 2 == 0 and needed == ro.source_frames(BIG_FRAMES, [(L, M, ro.taps(L, M)) for L, M in BIG_PLAIN])
    return needed + 1


def big_boundaries(rows=2 * BIG_WINDOWS, frames=BIG_FRAMES, source_frames=None):
    """buffer -> the element indices that are the named boundaries: elements 2^31 and 2^32, bytes 2^32, 2^33 (and 2^34, float32)"""
    source_frames = source_frames or big_source_frames()
    return {"int16": (frames, 2, [1 << 31, 1 << 32] + [(1 << b) // 2 for b in (32, 33)]),
            "float32": (frames, 4, [1 << 31, 1 << 32] + [(1 << b) // 4 for b in (32, 33, 34)]),
            "source": (source_frames, 2, [1 << 31, 1 << 32] + [(1 << b) // 2 for b in (32, 33)])}


def big_witness_windows(rows=2 * BIG_WINDOWS, frames=BIG_FRAMES, source_frames=None):
    """the windows (C = 2) whose rows are the 16 on each side of every boundary of every buffer, the straddling row, and the 16
    at both ends of the batch - sorted, unique"""
    ws = set(range(8)) | set(range(rows // 2 - 8, rows // 2))
    for pitch, _, elements in big_boundaries(rows, frames, source_frames).values():
        for e in elements:
            r = e // pitch
            ws |= {q // 2 for q in range(r - 16, r + 17)}
    return np.array(sorted(ws), dtype=np.int64)


# ---- rows and records through torch, on the CPU for rows with an acc and on the device for the identity bulk ----------------------------
def torch_dtype(name):
    import torch
    return {"int16": torch.int16, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16, "int64": torch.int64}[name]


def bit_view(t):
    """a tensor of any sample type as integers of its width: -0 and NaNs compare by their bits"""
    import torch
    return t if t.dtype in (torch.int16, torch.int64) else t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def old_pattern(e, name):
    """what an ADD run finds at element index e (an int64 tensor) of the output buffer: (e mod 251 - 125) / 128, a value of every
    float type"""
    import torch
    return ((e % 251 - 125).to(torch.float32) * 0.0078125).to(torch_dtype(name))


def placed_rows(f, le, o, gain, name, old=None):
    """mo.expected_rows over rows: f float32 [R, T], the plain run's float32 rows; (le, o) int64 [R], the CLIPPED span of each row
    (po.clipped); gain float32 [R]; old: None - STORE - or the rows before an ADD run, of the type -> the rows, of the type.  One
    float32 multiply, under ADD one float32 add, one rounding to the type: each a torch operation of its own."""
    import torch
    T = f.shape[1]
    t = torch.arange(T, device=f.device)[None, :]
    inside = (t >= o[:, None]) & (t < (o + le)[:, None])
    p = gain[:, None] * f.gather(1, (t - o[:, None]).clamp(0, T - 1))
    if old is not None:
        p = old.to(torch.float32) + p
    res = p.to(torch_dtype(name))
    return torch.where(inside, res, old if old is not None else torch.zeros((), dtype=res.dtype, device=f.device))


def row_records(v16, le, counts):
    """mo.expected_stats over rows: v16 int16 [R, T]; le int64 [R]; counts int64 [R] -> int64 [R, 4]"""
    import torch
    t = torch.arange(v16.shape[1], device=v16.device)[None, :]
    a = torch.where(t < le[:, None], v16.to(torch.int64).abs(), torch.zeros((), dtype=torch.int64, device=v16.device))
    return torch.stack([(a * a).sum(dim=1), a.sum(dim=1), a.max(dim=1).values, counts], dim=1)


def identity_counts(c_src, t_src, shift, le):
    """resample_output_count for L = M = 1 over tensors: 0 for c <= shift, else min(Le, c - shift), c = min(c_src, T_src)"""
    c = c_src.clamp(max=t_src)
    return ((c - shift).clamp(min=0)).minimum(le)


def rows_of_type(acc, name):
    """ro.convert as a CPU tensor of the type: acc int64 numpy [R, T]"""
    import torch
    bits = np.ascontiguousarray(ro.convert(acc, name))
    if name == "int16":
        return torch.from_numpy(bits)
    return torch.from_numpy(bits.view(np.int32 if name == "float32" else np.int16)).view(torch_dtype(name))


def run_expected(run, acc, le, o, gain, old, counts_full, counts_span):
    """kernel_expected over ROWS, vectorised, on the CPU: acc int64 numpy [R, T]; (le, o) int64 numpy [R], each row's clipped span;
    gain float32 numpy [R]; old: the rows before an ADD run, a CPU tensor of the type, or None; counts_*: int64 numpy [R] over the
    whole row and over the span -> (rows of the type or None, int64 records [R, 4] or None), CPU tensors"""
    import torch
    kind, name, flag = run
    R, T = acc.shape
    whole = torch.full((R,), T, dtype=torch.int64)
    if kind == "rows":
        return rows_of_type(acc, name), None
    if kind == "gain":
        return placed_rows(rows_of_type(acc, "float32"), torch.from_numpy(le), torch.from_numpy(o),
                           torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float32)), name, old if flag else None), None
    v16 = rows_of_type(acc, "int16")
    if flag:
        return None, row_records(v16, torch.from_numpy(le), torch.from_numpy(counts_span))
    return (None if name is None else rows_of_type(acc, name)), row_records(v16, whole, torch.from_numpy(counts_full))


def clipped_rows(spans, n, frames, channels):
    """po.clipped per ROW, vectorised: -> (le, o) int64 numpy [n * channels]; o is 0 where le is 0"""
    spans = np.asarray(spans, dtype=np.int64).reshape(n, 2)
    length, o = spans[:, 0].view(np.uint64), spans[:, 1].view(np.uint64)  # negative int64 values wrap
    room = np.uint64(frames) - np.minimum(o, np.uint64(frames))
    le = np.minimum(length, room).astype(np.int64)
    return np.repeat(le, channels), np.repeat(np.where(le > 0, spans[:, 1], 0), channels)
