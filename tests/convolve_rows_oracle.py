"""The convolve stage's C calls on hand-made source rows (AADHip_ConvolverRun, ...RunGain; include/aad_hip.h "reverberation") for
LARGE shapes, and the case tables of tests/test_gpu_convolve_geometry.py as pure functions, so that
tests/test_convolve_geometry_host.py can hold both with no GPU:

  expected_acc          acc of rows whose source row is given directly and whole - the row is the full pitch, so what lies behind
                        T_src is source like any other - by convolve_oracle.sums: element j = shift + n + d - k, zero outside the row;
  run_expected          what each of the ten FIR kernels of a convolver writes for given acc, scales, spans, gains and old rows,
                        through convolve_oracle.element_bits and resample_rows_oracle.placed_rows;
  recurrence            the closed form of the response [3, -2, 1] over an array namespace: numpy on the host, torch on the device;
  the tables            responses, lanes, the item-loop pairs, the 2^31 shape, the 4 GiB placements.

TEST INFRASTRUCTURE (tests/ only).  No torch at module level, no library."""
import itertools

import numpy as np

import convolve_matrix as cm
import convolve_oracle as co
import resample_rows_oracle as rr

TILE = 4096          # outputs of one workgroup's tile (aad_convolve.h kConvolveTile)
BLOCK = 256          # outputs of one accumulator tile (kConvolveBlock)
STEP_TAPS = 64       # taps of a k-step (kConvolveStepTaps)
PIECE_STEPS = 64     # k-steps between two stagings of the span (kConvolvePieceSteps)
GRID = 1 << 20       # workgroups of the largest grid (convolve::grid): the item loop takes the rest
DTYPES = ("int16", "float32", "float16", "bfloat16")
FLOATS = DTYPES[1:]
NO_RESPONSE = co.NO_RESPONSE

torch_dtype, bit_view, old_pattern, placed_rows, clipped_rows = rr.torch_dtype, rr.bit_view, rr.old_pattern, rr.placed_rows, rr.clipped_rows


def steps(K):
    """aad_convolve.h convolve_steps"""
    return (K + 15 + STEP_TAPS - 1) // STEP_TAPS


def pieces(K):
    return -(-steps(K) // PIECE_STEPS)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------
# (kind, sample type, ADD): the ten FIR kernels a convolver launches
RUNS = [("rows", t, False) for t in DTYPES] + [("gain", t, add) for t in FLOATS for add in (False, True)]


def run_id(run):
    kind, name, add = run
    return "gain-%s-%s" % (name, "add" if add else "store") if kind == "gain" else "rows-%s" % name


def kernel_of(run):
    """the record of tests/convolve_matrix.py that a run launches: (kernel, template arguments)"""
    kind, name, add = run
    st = {"int16": cm.INT16, "float32": cm.FLOAT32, "float16": cm.FLOAT16, "bfloat16": cm.BFLOAT16}[name]
    return ("convolve_rows_kernel", (st,)) if kind == "rows" else ("convolve_rows_gain_kernel", (st, cm.ADD if add else cm.STORE))


# ---- the FIR on given rows -------------------------------------------------------------------------------------------------------------
def lane_table(lanes):
    """[N, 2] of (response, shift) as the unsigned 32-bit values the device reads"""
    return np.asarray(lanes, dtype=np.int64).reshape(-1, 2) & 0xFFFFFFFF


def device_lanes(lanes):
    """the int32 [N, 2] array whose bits are the lane table"""
    return np.ascontiguousarray(lane_table(lanes).astype(np.uint32).view(np.int32))


def expected_acc(src_rows, lanes, responses, frames, channels):
    """src_rows: int16 [N * C, pitch], every row whole; lanes: [N, 2] of (response, shift), response 0xFFFFFFFF or >= R: none;
    responses: [(taps, q, delay)] -> int64 acc [N, C, frames]"""
    lanes = lane_table(lanes)
    n = len(lanes)
    src_rows = np.asarray(src_rows)
    assert src_rows.ndim == 2 and src_rows.shape[0] == n * channels
    acc = np.zeros((n * channels, frames), dtype=np.int64)
    for w, (r, shift) in enumerate(lanes.tolist()):
        if r >= len(responses):
            continue
        taps, _, delay = responses[r]
        for c in range(channels):
            acc[w * channels + c] = co.sums(src_rows[w * channels + c], shift, frames, taps, delay)
    return acc.reshape(n, channels, frames)


def lane_scales(lanes, responses):
    """q of every window's response, 0 without one"""
    return np.array([responses[r][1] if r < len(responses) else 0 for r in lane_table(lanes)[:, 0].tolist()], dtype=np.int64)


def rows_of_type(acc, qs, name):
    """co.element_bits as a CPU tensor of the type: acc int64 numpy [R, T], qs [R] the scale of each row"""
    import torch
    bits = np.empty(acc.shape, dtype=np.uint32 if name == "float32" else np.uint16)
    qs = np.asarray(qs, dtype=np.int64)
    for q in np.unique(qs).tolist():
        bits[qs == q] = co.element_bits(acc[qs == q], q, name)
    if name == "int16":
        return torch.from_numpy(bits.view(np.int16))
    return torch.from_numpy(bits.view(np.int32 if name == "float32" else np.int16)).view(torch_dtype(name))


def run_expected(run, acc, qs, le, o, gain, old):
    """one run over ROWS, on the CPU: acc int64 numpy [R, T]; qs [R]; (le, o) int64 numpy [R], each row's clipped span
    (clipped_rows); gain float32 numpy [R]; old: the rows before an ADD run, a CPU tensor of the type, or None -> a CPU tensor of
    the type.  The gain runs take the span and the gain, the plain runs the whole row."""
    import torch
    kind, name, add = run
    if kind == "rows":
        return rows_of_type(acc, qs, name)
    return placed_rows(rows_of_type(acc, qs, "float32"), torch.from_numpy(np.ascontiguousarray(le)), torch.from_numpy(np.ascontiguousarray(o)),
                       torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float32)), name, old if add else None)


def spans_for(n, frames):
    """spans in output frames: whole, across elements 4096 and 8192 where the row has them, odd and even offsets, clipped, empty,
    and (T / 2, 5) - at T = 9 the span (4, 5)"""
    T = frames
    kinds = [(T, 0), (T - T // 4, T // 5 - (T // 5) % 2 + 1), (0, 0), (5, 0), (T, 1), (10, T - 1), (10, T), (T // 2, 7), (T // 2, 8),
             (T - 9, 9), (-1, 3), (T // 2, 5)]
    return np.array(kinds, dtype=np.int64)[np.arange(n) % len(kinds)]


def bulk_gains(rng, n):
    """exact powers of two of both signs: g f is exact for every element of every float type's range here"""
    return (2.0 ** rng.integers(-3, 3, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


def source_rows(rng, rows, pitch):
    """random int16 rows with the rails sprinkled in"""
    x = rng.integers(-32768, 32768, size=(rows, pitch)).astype(np.int16)
    rail = rng.integers(0, 24, size=x.shape)
    x[rail == 0], x[rail == 1] = 32767, -32768
    return x


def decaying(rng, K, peak, scale=1.0):
    """a float response of K taps: 1.0 * scale at `peak`, a decaying tail of random taps around it"""
    h = rng.uniform(-0.9, 0.9, size=K) * np.exp(-np.arange(K) * (6.0 / K))
    h[peak] = 1.0
    return (h * scale).astype(np.float32)


def quantised(hs, delays):
    """[(taps int64, q, delay)] as the library must quantise them (convolve_oracle.quantise)"""
    out = []
    for h, d in zip(hs, delays):
        taps, q, delay = co.quantise(h, d)
        out.append((taps.astype(np.int64), q, delay))
    return out


# ---- the closed form of [3, -2, 1] -------------------------------------------------------------------------------------------------------
RECURRENCE_RESPONSE = [3.0, -2.0, 1.0]
RECURRENCE_TAPS, RECURRENCE_Q, RECURRENCE_DELAY = (24576, -16384, 8192), 13, 0  # what the library must quantise it to
UNIT_TAPS, UNIT_Q = (16384,), 14                                                # and {1.0}: the row is the source slice


def recurrence(x, shift, frames, lo=0, hi=None, xp=np, **where):
    """v[n] = 3 x[j] - 2 x[j - 1] + x[j - 2], j = shift + n, for lo <= n < hi (hi: frames), x a 1-d integer array of the namespace
    xp read as zero outside itself -> int64 [hi - lo] of xp.  acc[n] = 8192 v[n] under RECURRENCE_TAPS, so with q = 13 the int16
    element is clamp(v) (recurrence_int16) and the float32 element v * 2^-15, exact: |v| <= 6 * 32768 < 2^24.
    where: what xp.zeros takes to put the result beside x (device=...)."""
    hi = frames if hi is None else hi
    assert 0 <= lo <= hi <= frames
    size = int(x.shape[0])
    first = shift + lo - 2                  # the source element under p[0]; p[i] = x[first + i], zero outside the row
    p = xp.zeros(hi - lo + 2, dtype=xp.int64, **where)
    a, b = max(first, 0), min(first + hi - lo + 2, size)
    if b > a:
        p[a - first:b - first] = x[a:b]
    return 3 * p[2:] - 2 * p[1:-1] + p[:-2]


def recurrence_int16(v, xp=np):
    return xp.clip(v, -32768, 32767)


# ---- a, b. placement and the surplus behind T_src ------------------------------------------------------------------------------------------
PLACE_FRAMES = (257, 1025)
PLACE_TAPS = (1, 64, 65, 1000, 4200)
PLACE_DELAYS = (0, 0, 32, 333, 1400)
PLACE_SCALES = (1.0, 0.3, 3.0, 200.0, 1.0)  # q = 14, 15, 13, 7, 14
PLACE_EXTRAS = (0, 1, 37)
SURPLUS = 37                                 # the pitch of test_shift_past_the_lead is T_src + SURPLUS


def place_responses():
    rng = np.random.default_rng(4200)
    return [decaying(rng, K, d, s) for K, d, s in zip(PLACE_TAPS, PLACE_DELAYS, PLACE_SCALES)], list(PLACE_DELAYS)


def leads(responses):
    return [len(taps) - 1 - d for taps, _, d in responses]


def place_lanes(responses):
    """per response the shifts 0, 1, lead / 2 and lead - never past the lead: no output reads behind T_src - and one window
    without a response"""
    lanes = [(r, s) for r, lead in enumerate(leads(responses)) for s in sorted({0, min(1, lead), lead // 2, lead})]
    return np.array(lanes + [(NO_RESPONSE, 7)], dtype=np.int64)


def past_lead_lanes(responses, pitch):
    """per response the shifts lead + 1, lead + 36, lead + 37, the pitch, 2^31 - 1, 2^31 and 2^32 - 1"""
    lanes = [(r, s) for r, lead in enumerate(leads(responses))
             for s in (lead + 1, lead + SURPLUS - 1, lead + SURPLUS, pitch, (1 << 31) - 1, 1 << 31, (1 << 32) - 1)]
    return np.array(lanes, dtype=np.int64)


def pitched(rows, t_src, extra):
    """int16 rows [R, T_src] -> [R, T_src + extra]: the surplus filled with the rails, +32767 and -32768 in turn"""
    out = np.empty((rows.shape[0], t_src + extra), dtype=np.int16)
    out[:, :t_src] = rows
    out[:, t_src:] = np.where((np.arange(extra)[None, :] + np.arange(rows.shape[0])[:, None]) % 2 == 0, 32767, -32768)
    return out


# ---- c. the item loop --------------------------------------------------------------------------------------------------------------------
ITEM_FRAMES = 9
ITEM_EXTRA = 1024                      # E: the workgroups that take a second item
ITEM_KINDS = (None, 1, 40, 1000, 4082)  # no response, or the taps of response k: 1, 1, 16 and 65 k-steps - the last two pieces


def item_rows(extra=ITEM_EXTRA):
    return GRID + extra


def item_responses():
    """response 0 is {1.0}, the bulk's; response k > 0 has ITEM_KINDS[k] taps"""
    rng = np.random.default_rng(4082)
    hs = [np.array([1.0], dtype=np.float32), np.array([-0.75], dtype=np.float32)]
    hs += [decaying(rng, K, K // 3, s) for K, s in zip(ITEM_KINDS[2:], (3.0, 0.3, 1.0))]
    return hs, [0, 0] + [K // 3 for K in ITEM_KINDS[2:]]


def item_pairs(extra=ITEM_EXTRA):
    """[extra, 2]: the kinds of rows b and 2^20 + b of workgroup b < extra - every ordered pair in turn"""
    pairs = list(itertools.product(range(len(ITEM_KINDS)), repeat=2))
    return np.array([pairs[b % len(pairs)] for b in range(extra)], dtype=np.int64)


def item_lanes(responses, seed=1 << 20, extra=ITEM_EXTRA):
    """-> (lanes [rows, 2], the designed rows): every row the unit response with shift row mod 4, but rows b and 2^20 + b of
    workgroup b < extra, which take their kinds from item_pairs and a shift in 0 .. lead + 2"""
    rng = np.random.default_rng(seed)
    rows = item_rows(extra)
    lanes = np.empty((rows, 2), dtype=np.int64)
    lanes[:, 0], lanes[:, 1] = 0, np.arange(rows) % 4
    lead = leads(responses)
    pairs = item_pairs(extra)
    for j in range(2):
        for b in range(extra):
            k = int(pairs[b, j])
            lanes[j * GRID + b] = (NO_RESPONSE, 7) if k == 0 else (k, rng.integers(0, lead[k] + 3))
    return lanes, np.concatenate([np.arange(extra), GRID + np.arange(extra)])


# ---- d. the 2^31 limit -------------------------------------------------------------------------------------------------------------------
LIMIT_FRAMES = (1 << 31) + TILE + 77  # the last tile has 77 outputs: one block
LIMIT_SHIFTS = (2, 0)
LIMIT_OFFSETS = (1, TILE + 1)         # the spans (T - o, o) of the gain run


# ---- e. past 4 GiB -----------------------------------------------------------------------------------------------------------------------
BIG_FRAMES = TILE + 3  # a full tile and a tile of three outputs: waves 1 - 3 have no block
BIG_WINDOWS = 524400   # C = 2: 1 048 800 rows, 2 097 600 items
BIG_TAPS = (1, 64, 65, 17)
BIG_WITNESSES = 256


def big_pitch():
    """T_src = T + 64 = 4163 and two more: above T_src, and odd, so the source rows alternate 4-byte alignment"""
    return BIG_FRAMES + max(BIG_TAPS) - 1 + 2


def big_responses():
    rng = np.random.default_rng(4099)
    hs = [np.array([1.0], dtype=np.float32)] + [decaying(rng, K, d, s) for K, d, s in zip(BIG_TAPS[1:], (0, 64, 5), (1.0, 3.0, 0.3))]
    return hs, [0, 0, 64, 5]


def big_boundaries(rows=2 * BIG_WINDOWS):
    """buffer -> (pitch, the element indices that are byte or element boundaries): bytes 2^32 (and 2^33, 2^34), elements 2^31, 2^32"""
    return {"int16": (BIG_FRAMES, [1 << 31, 1 << 32]), "float32": (BIG_FRAMES, [1 << 30, 1 << 31, 1 << 32]),
            "source": (big_pitch(), [1 << 31, 1 << 32])}


def big_witness_windows(rows=2 * BIG_WINDOWS):
    """256 windows (C = 2): the rows 16 on each side of every boundary of every buffer with the straddling row, the 8 windows at both
    ends of the batch, and a seeded sample of the rest - sorted, unique"""
    ws = set(range(8)) | set(range(rows // 2 - 8, rows // 2))
    for pitch, elements in big_boundaries(rows).values():
        for e in elements:
            r = e // pitch
            ws |= {q // 2 for q in range(r - 16, r + 17)}
    rest = np.setdiff1d(np.arange(rows // 2), np.array(sorted(ws)))
    more = np.random.default_rng(256).choice(rest, size=BIG_WITNESSES - len(ws), replace=False)
    return np.sort(np.concatenate([np.array(sorted(ws), dtype=np.int64), more.astype(np.int64)]))
