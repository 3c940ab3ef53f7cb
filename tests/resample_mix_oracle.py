"""Resampled rows with a gain, spans and level statistics (include/aad_hip.h, AADHip_ResamplerRunGain / AADHip_ResamplerRunStats)
restated on the CPU, on top of tests/resample_oracle.py (acc and its conversions), tests/window_placed_oracle.py (spans: Le, the
placement, STORE's zeros) and tests/window_gain_oracle.py (the multiply, the add and the one rounding of the type, through torch):

    f      = fl32(acc) * 2^-29                                   the plain run's float32 row, +0 without a bank
    rows   = placed_expected(f, spans, gain, dtype, old)         window decode with spans, f in place of its value
    v      = clamp((acc + 8192) >> 14)                            the plain run's int16 row
    record = sum v^2, sum |v|, max |v| over n < Le, count = #{n < Le : first_frame + (n M) div L < num_samples[stream]}

`count` is computed twice - the closed form the library uses, over the source batch's own count, and a brute force over n from
the stream table - and the two must agree.

The WITNESSES are elements on which a wrong implementation gives another value than the definition:
  (a) "fused":  fl(old + g * f) in one rounding - a fused multiply-add - instead of fl32(old + fl32(g * f));
  (b) "double": g * f rounded straight to float16 / bfloat16, its float32 rounding skipped;
  (c) "exact":  g * (acc * 2^-29) with the exact acc where the definition multiplies fl32(acc), which differs once |acc| > 2^24.
All three are evaluated in float64 and only where float64 is exact: a product of two float32 values has 48 bits; a sum is taken
with its rounding error (two_sum) and an element whose sum is inexact is not reported; a float32 result rounded from an exact
float64 value rounds once.  craft() searches gains (and old values) that make one given element a witness, directed at the
type's rounding ties: random gains find such elements for float32 alone.

TEST INFRASTRUCTURE (tests/ only)."""
import numpy as np

import resample_oracle as ro
import window_gain_oracle as go
import window_placed_oracle as po
from window_stats_oracle import stats_of_rows, window_counts

U64 = 1 << 64
KINDS = ("fused", "double", "exact")


# ---- rows --------------------------------------------------------------------------------------------------------------------------
def float_rows(acc):
    """int64 acc [N, C, T] -> the plain run's float32 rows"""
    return ro.convert(acc, "float32").view(np.float32)


def expected_rows(acc, spans, gain, name, old_bits=None):
    """acc: int64 [N, C, T], zeros for a window without a bank; spans: int [N, 2] in output frames or None; gain: float32 [N] or
    None; old_bits: None - STORE - or the rows' bit patterns before an ADD run -> the rows' bit patterns after the run"""
    return po.placed_expected(float_rows(acc), spans, gain, name, old_bits)


# ---- records -----------------------------------------------------------------------------------------------------------------------
def output_count(c_src, source_frames, shift, L, M, le):
    """the closed form of aad_resample.h's resample_output_count"""
    c = min(int(c_src), int(source_frames))
    if c <= shift:
        return 0
    return min(int(le), -(-(c - shift) * L // M))


def output_count_brute(c_src, source_frames, shift, L, M, le):
    c = min(int(c_src), int(source_frames))
    return sum(1 for n in range(int(le)) if shift + n * M // L < c)


def expected_counts(lengths, windows, variant, select, banks, frames, spans):
    """int64 [N]: per window the closed form over the source batch's count - window decode's count of the source window
    AADHip_ResamplerResolve writes - held against the brute force over the stream table; 0 without a bank"""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    select = np.asarray(select).reshape(len(select), -1)
    t_src = ro.source_frames(frames, [(L, M, h.shape[1]) for L, M, h in banks])
    spans_le = po.clipped(spans, len(windows), frames)
    out = np.zeros(len(windows), dtype=np.int64)
    for w, (s, first) in enumerate(windows.tolist()):
        v = 0 if variant is None else int(variant[w]) % U64
        s, first = s % U64, first % U64
        if s >= select.shape[0] or v >= select.shape[1] or select[s][v] == ro.NO_BANK:
            continue
        L, M, h = banks[int(select[s][v])]
        src_first, shift = ro.resolve(first, h.shape[1])
        c_src = int(window_counts(lengths, np.array([[s, src_first]], dtype=np.uint64).view(np.int64), t_src)[0])
        le = spans_le[w][0]
        closed = output_count(c_src, t_src, shift, L, M, le)
        brute = sum(1 for n in range(le) if s < len(lengths) and first + n * M // L < int(lengths[s]))
        assert closed == brute == output_count_brute(c_src, t_src, shift, L, M, le), (w, s, first, closed, brute)
        out[w] = closed
    return out


def expected_stats(acc, spans, counts):
    """acc: int64 [N, C, T]; counts: expected_counts -> int64 [N, C, 4] over each window's first Le frames"""
    rows16 = np.array(ro.convert(acc, "int16"))
    n, _, frames = rows16.shape
    for w, (le, _) in enumerate(po.clipped(spans, n, frames)):
        rows16[w, :, le:] = 0
    return stats_of_rows(rows16, counts)


# ---- witnesses ---------------------------------------------------------------------------------------------------------------------
def two_sum(a, b):
    """float64 a + b and whether it is exact"""
    s = a + b
    bb = s - a
    return s, ((a - (s - bb)) + (b - bb)) == 0


def _f32(x):
    """float64 -> the nearest float32 value, as float64 (one rounding of the value given, subnormals kept)"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _narrow(x32, name):
    """float32 values (as float64) -> the type's nearest values"""
    return x32 if name == "float32" else go.round_f64(x32, name)


def differs(kind, name, acc, gain, old=None):
    """acc: int array; gain: float32 values; old: values of the type, "fused" alone (arrays that broadcast) -> bool array: the
    wrong implementation of `kind` gives another value of the type than the definition, provably"""
    acc = np.asarray(acc, dtype=np.int64)
    g = np.asarray(gain, dtype=np.float32).astype(np.float64)
    f = acc.astype(np.float32).astype(np.float64) * 2.0 ** -29
    product = g * f  # exact: 24 x 24 bits
    p = _f32(product)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == "fused":
            old = np.asarray(old, dtype=np.float64)
            right = _narrow(_f32(old + p), name)  # a float64 sum of two float32 values rounds to float32 as the exact sum does
            s, exact = two_sum(old, product)
            return exact & (_narrow(_f32(s), name) != right)
        right = _narrow(p, name)
        if kind == "double":
            if name == "float32":
                return np.zeros(np.broadcast(acc, g).shape, dtype=bool)
            return go.round_f64(product, name) != right
        assert kind == "exact"
        hi, lo = acc >> 12, acc & 4095  # g * acc in two exact pieces: 24 + 19 and 24 + 12 bits
        s, exact = two_sum(g * (hi.astype(np.float64) * 4096.0), g * lo.astype(np.float64))
        return exact & (_narrow(_f32(s * 2.0 ** -29), name) != right)


def witnesses(acc, gain, name, old_bits=None):
    """acc: int64 [N, C, T]; gain: float32 [N]; old_bits: the rows before an ADD run, or None: a STORE run -> {kind: bool
    [N, C, T]}: "fused" under ADD, "double" and "exact" under STORE"""
    g = np.asarray(gain, dtype=np.float32)[:, None, None]
    if old_bits is not None:
        old = go.from_bits(old_bits, name).float().numpy().astype(np.float64)
        return {"fused": differs("fused", name, acc, g, old)}
    return {kind: differs(kind, name, acc, g) for kind in ("double", "exact")}


def _ulp(value, name):
    p, emin = go.FORMATS[name]
    _, e = np.frexp(np.abs(value))
    return np.ldexp(1.0, np.maximum(e - 1, emin) - p + 1)


def craft(kind, name, accs, seed=0):
    """accs: the int acc values of one window's candidate elements -> (index into accs, gain float32, old value or None) that
    make the element a witness of `kind` for type `name`.  Directed: the gains whose product - "fused": old + product - lies
    next to a rounding tie of the type (float32 for "exact" and "fused" on float32 rows: any value), 257 neighbouring float32
    gains around each of 64 ties per element."""
    rng = np.random.default_rng([seed, KINDS.index(kind), len(name)])
    accs = np.asarray(accs, dtype=np.int64)
    f = accs.astype(np.float32).astype(np.float64) * 2.0 ** -29
    inexact = accs.astype(np.float32).astype(np.int64) != accs
    order = np.argsort(-np.abs(accs) * (inexact if kind == "exact" else 1), kind="stable")[:16]  # the loudest, "exact": that float32 rounds
    steps = np.arange(-128, 129, dtype=np.float64)
    for i in order.tolist():
        if f[i] == 0:
            continue
        ulp = _ulp(f[i], "float32" if name == "float32" else name)
        ties = (np.floor(np.abs(f[i]) / ulp) + rng.integers(-40, 40, size=64) + 0.5) * ulp  # between two values of the type
        old = None
        if kind == "fused":
            old = go.round_f64(rng.uniform(-0.5, 0.5, size=64) * np.abs(f[i]), "bfloat16")  # a value of every type
            ties = ties - old
        centre = (ties / f[i]).astype(np.float32)
        gains = (centre.astype(np.float64)[:, None] + steps[None, :] * _ulp(centre.astype(np.float64), "float32")[:, None])
        gains = gains.astype(np.float32)
        hit = differs(kind, name, accs[i], gains, None if old is None else old[:, None])
        hit &= np.isfinite(gains) & (gains != 0)
        at = np.argwhere(hit)
        if len(at):
            t, k = at[0]
            return i, np.float32(gains[t, k]), None if old is None else float(old[t])
    raise AssertionError("no %s witness for %s among %d elements" % (kind, name, len(accs)))
