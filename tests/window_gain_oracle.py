"""Window decode with a per-window gain (include/aad_hip.h, AADHip_WindowDecodePlanRunGain) restated through torch on the CPU:

    STORE  (gain[:, None, None] * row_float32).to(dtype)
    ADD    (out.float() + gain[:, None, None] * row_float32).to(dtype)

row_float32 being the float32 rows of tests/window_oracle.py / tests/channel_mix_oracle.py, every element of [N, C, T], padding
included.  torch's CPU multiply and add are two kernels (two roundings, subnormals kept) and its conversions round once.

The WITNESSES are inputs on which a wrong implementation gives other bits than the definition: a product that rounds differently
to float16 / bfloat16 when its float32 rounding is skipped, an old value that gives another float32 when multiply and add are
fused, a subnormal product that rounds twice when the gain is applied before the 2^-15.  They are found with float64 arithmetic
in numpy (exact here: a 24-bit gain times a 16-bit sample, sums of nearby magnitudes) and each is confirmed with
fractions.Fraction by tests/test_window_gain_host.py - never by the code under test.  The witness samples travel as the header
samples of a crafted stream's first two blocks (a block's four header samples are stored verbatim), eight values in all, and the
windows that start on those blocks carry the witness gains.  Header samples are stored one by one; vector_witnesses() finds
witnesses of the same kinds on the samples behind them, which leave by the kernels' 16-element vector stores (see there).

TEST INFRASTRUCTURE (tests/ only)."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

DTYPES = ("float32", "float16", "bfloat16")
FORMATS = {"float32": (24, -126), "float16": (11, -14), "bfloat16": (8, -126)}  # significand bits, exponent of the smallest normal

# the header samples of the witness stream's blocks 0 and 1: magnitudes from 2^10 up, so that products and old values lie close
WITNESS_SAMPLES = (12345, -7777, 30001, 1023, -20481, 4097, -32768, 2731)


def torch_dtype(name):
    import torch
    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[name]


def bits_of(t):
    """torch tensor of a DTYPES type -> numpy array of its bit patterns (uint32 / uint16)"""
    import torch
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(bits, name):
    """numpy array of bit patterns -> torch tensor of the type"""
    import torch
    bits = np.ascontiguousarray(bits)
    if name == "float32":
        return torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch_dtype(name))


def gain_expected(rows32, gain, name, old_bits=None):
    """rows32: float32 [N, C, T]; gain: float32 [N] (None: every gain is 1); old_bits: None - STORE - or the bit patterns the rows
    held - ADD -> the bit patterns of the rows after the run"""
    import torch
    rows = torch.from_numpy(np.ascontiguousarray(rows32, dtype=np.float32))
    g = torch.ones(rows.shape[0], dtype=torch.float32) if gain is None else torch.from_numpy(np.ascontiguousarray(gain, dtype=np.float32))
    p = g[:, None, None] * rows
    if old_bits is not None:
        p = from_bits(old_bits, name).float() + p
    return bits_of(p.to(torch_dtype(name)))


# ---- exact arithmetic --------------------------------------------------------------------------------------------------------------
def round_fraction(x, name):
    """Fraction -> the Fraction of the type's nearest value, ties to even, subnormals kept (no overflow handling)"""
    p, emin = FORMATS[name]
    x = Fraction(x)
    if x == 0:
        return x
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, emin) - p + 1)
    n = a / ulp
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r % 2 == 1):
        r += 1
    return (r * ulp) if x > 0 else -(r * ulp)


def round_f64(x, name):
    """float64 array of exactly known values -> float64 array of the type's nearest values (the vectorised round_fraction)"""
    p, emin = FORMATS[name]
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)  # |x| in [2^(e-1), 2^e)
    ulp = np.ldexp(1.0, np.maximum(e - 1, emin) - p + 1)
    return np.rint(x / ulp) * ulp  # rint: ties to even; the division and the product are by a power of two


def _f(sample):
    return np.asarray(sample, dtype=np.float64) / 32768.0


def witnesses():
    """-> dict of witness lists over WITNESS_SAMPLES (at least 8 each, at most 16):
      "double_float16", "double_bfloat16": (g, sample) with fl32(g * f) rounded to the type != the exact g * f rounded once;
      "fused": (old, g, sample), old a bfloat16 value (so a value of every type), with fl32(old + fl32(g * f)) != the exact
               old + g * f rounded once to float32;
      "order": (g, sample), g near 2^-134, with fl32(g * f) != fl32(fl32(sample * g) * 2^-15)"""
    rng = np.random.default_rng(20250)
    s = np.array(WITNESS_SAMPLES, dtype=np.float64)[None, :]
    out = {}
    g = rng.uniform(-2.0, 2.0, size=400000).astype(np.float32).astype(np.float64)[:, None]
    exact = g * _f(s)
    p32 = round_f64(exact, "float32")
    for name in ("float16", "bfloat16"):
        i, j = np.nonzero(round_f64(p32, name) != round_f64(exact, name))
        out["double_" + name] = [(np.float32(g[a, 0]), WITNESS_SAMPLES[b]) for a, b in zip(i[:16], j[:16])]
    g = rng.uniform(-2.0, 2.0, size=64).astype(np.float32).astype(np.float64)[:, None]
    old = round_f64(rng.uniform(-2.0, 2.0, size=g.shape) * rng.choice([1.0, 0.25], size=g.shape), "bfloat16")
    exact = g * _f(s)
    two = round_f64(old + round_f64(exact, "float32"), "float32")
    i, j = np.nonzero(two != round_f64(old + exact, "float32"))
    pick = rng.permutation(len(i))[:16]
    out["fused"] = [(np.float32(old[a, 0]), np.float32(g[a, 0]), WITNESS_SAMPLES[b]) for a, b in zip(i[pick], j[pick])]
    g = (np.ldexp(1.0, -134) * rng.uniform(1.0, 2.0, size=4000)).astype(np.float32).astype(np.float64)[:, None]
    once = round_f64(g * _f(s), "float32")
    twice = round_f64(round_f64(s * g, "float32") * 2.0 ** -15, "float32")
    i, j = np.nonzero(once != twice)
    out["order"] = [(np.float32(g[a, 0]), WITNESS_SAMPLES[b]) for a, b in zip(i[:16], j[:16])]
    return out


def witness_windows(stream, spb):
    """-> (windows int64 [W, 2], gains float32 [W], olds: list of (window, t, old float32)): one window per witness, starting on the
    block of `stream` whose header holds the witness sample (element t of every row of the window is that sample, the crafted
    stream having the same history in all its channels); the "fused" windows want `old` planted there before an ADD run"""
    w = witnesses()
    windows, gains, olds = [], [], []
    for key in ("double_float16", "double_bfloat16", "order"):
        for g, sample in w[key]:
            k = WITNESS_SAMPLES.index(sample)
            windows.append((stream, (k // 4) * spb))
            gains.append(g)
    for old, g, sample in w["fused"]:
        k = WITNESS_SAMPLES.index(sample)
        olds.append((len(windows), k % 4, old))
        windows.append((stream, (k // 4) * spb))
        gains.append(g)
    return np.array(windows, dtype=np.int64), np.array(gains, dtype=np.float32), olds


# ---- witnesses on the vector path --------------------------------------------------------------------------------------------------
# The header witnesses above are a block's first four samples: WindowRow::one() stores them one by one.  Every other sample of a
# whole block leaves through WindowRow::chunk(): sixteen elements at a time, pairs packed into one word, the old values of an ADD
# run loaded as 16-byte vectors.  These witnesses sit there, on the row values the decode itself produces.
VECTOR_KINDS = ("double_float16", "double_bfloat16", "fused", "order")
CHUNK, TAPS = 16, 4

# kind: see witnesses(); window: the index of the candidate window; channel, t: the row element (t a crop index);
# old: None, or per row of the element - one row, or the two twin rows of a mono source in a to-stereo run - the old value of "fused"
VectorWitness = namedtuple("VectorWitness", "kind window channel t gain olds")


def chunk_elements(spb, le):
    """the crop indices that leave through chunk() in a window that starts on a block boundary of a complete block inside the
    stream: t in [4, 4 + 16 m), m = min((spb - 4) // 16, (Le - 4) // 16) whole chunks behind the four header samples"""
    m = max(min((int(spb) - TAPS) // CHUNK, (int(le) - TAPS) // CHUNK), 0)
    return range(TAPS, TAPS + CHUNK * m)


def chunk_class(t):
    """0 .. 3: the half of the packed word (even / odd t - 4) + 2 * the put8 call of the chunk ((t - 4) % 16 < 8 or not)"""
    return (t - TAPS) % 2 + 2 * ((t - TAPS) % CHUNK >= 8)


# gains of one batch of the search, batches at the most: about 100 000 gains for bfloat16, whose witnesses are the rarest; a product
# of k bits in units of 2^-149 is an order witness about once in 2^(25 - k) gains, so the quiet streams want many
SEARCH = {"double_float16": (5000, 4), "double_bfloat16": (20000, 5), "fused": (1000, 4), "order": (4000, 8)}


def _hits(kind, f, scale, rng):
    """f: float64 [E], row values -> (gains float64 [G], olds float64 [G] or None, hit matrix bool [G, E]) of the first batch
    of gains with a hit, or of the last batch"""
    size, batches = SEARCH[kind]
    for _ in range(batches):
        g, old, hit = _hits_of_batch(kind, f, scale, rng, size)
        if hit.any():
            break
    return g, old, hit


def _hits_of_batch(kind, f, scale, rng, size):
    if kind in ("double_float16", "double_bfloat16"):
        name = kind[len("double_"):]
        g = rng.uniform(-2.0, 2.0, size=size).astype(np.float32).astype(np.float64)
        exact = g[:, None] * f[None, :]
        p32 = exact.astype(np.float32).astype(np.float64)
        maybe = p32 != exact  # a product that float32 holds exactly rounds once either way
        hit = np.zeros(exact.shape, dtype=bool)
        hit[maybe] = round_f64(p32[maybe], name) != round_f64(exact[maybe], name)
        return g, None, hit
    if kind == "fused":
        # |g| >= 1/4 and |old| < 2: old + g * f spans fewer than 53 bits, float64 holds it exactly
        g = (rng.uniform(0.25, 2.0, size=size) * rng.choice([-1.0, 1.0], size=size)).astype(np.float32).astype(np.float64)
        old = round_f64(rng.uniform(-1.9, 1.9, size=g.shape) * rng.choice([1.0, 0.25], size=g.shape), "bfloat16")
        exact = g[:, None] * f[None, :]
        two = round_f64(old[:, None] + round_f64(exact, "float32"), "float32")
        return g, old, two != round_f64(old[:, None] + exact, "float32")
    assert kind == "order"
    g = (np.ldexp(1.0, -134) * rng.uniform(1.0, 2.0, size=size)).astype(np.float32).astype(np.float64)
    s = f * scale  # the integer the decoder holds
    once = round_f64(g[:, None] * f[None, :], "float32")
    twice = round_f64(round_f64(s[None, :] * g[:, None], "float32") / scale, "float32")
    return g, None, once != twice


def _second_old(f, g, first, rng):
    """another bfloat16 old value under which (g, f) is a "fused" witness: the twin row's"""
    old = round_f64(rng.uniform(-1.9, 1.9, size=4096) * rng.choice([1.0, 0.25], size=4096), "bfloat16")
    exact = g * f
    two = round_f64(old + round_f64(exact, "float32"), "float32")
    good = old[(two != round_f64(old + exact, "float32")) & (old != first)]
    if not len(good):
        raise AssertionError("no second old value for the twin row of a fused witness")
    return float(good[0])


def vector_witnesses(rows32, windows, spbs, les=None, scale=32768.0, twins=None, seed=20251):
    """rows32: float32 [N, C, T], the oracle's rows of N candidate windows, each starting on a block boundary of a complete,
    untruncated block that lies inside its stream's samples; windows: their [N, 2] table (the seed of a window's search comes from it);
    spbs: samples per block of each window's stream; les: the clipped span length of each (None: T); scale: 2^15, 2^16 for the
    rows of a down-mix, which hold (L + R) * 2^-16 - one value, or one per window; twins: per window, whether the rows are the two
    copies of a mono source.
    -> list of VectorWitness: per window and kind four, one in each chunk_class, the channel rotating; "fused" with its old
    values.  The search is over all elements of the class at once, in float64 as witnesses(), deterministic; a class that comes up
    empty raises - there is no run without a witness.  tests/test_window_gain_host.py confirms each with fractions.Fraction."""
    rows32 = np.asarray(rows32, dtype=np.float32)
    n, channels, frames = rows32.shape
    out = []
    for w in range(n):
        le = frames if les is None else int(les[w])
        ts = np.array(chunk_elements(spbs[w], le), dtype=np.int64)
        if len(ts) < 2 * CHUNK:
            raise AssertionError("window %d: fewer than two whole chunks (spb %d, Le %d)" % (w, spbs[w], le))
        twin = bool(twins[w]) if twins is not None else False
        rng = np.random.default_rng([seed, int(windows[w][0]) % (1 << 32), int(windows[w][1]) % (1 << 32)])
        for ki, kind in enumerate(VECTOR_KINDS):
            for cls in range(4):
                mine = ts[chunk_class(ts) == cls]
                found = None
                for turn in range(channels):  # the wanted channel first, the others when its elements give nothing
                    c = (w + ki + cls + turn) % channels
                    f = rows32[w, c, mine].astype(np.float64)
                    loud = np.argsort(-np.abs(f), kind="stable")[:16]  # the sixteen largest: the most significant bits to lose
                    g, old, hit = _hits(kind, f[loud], float(scale[w]) if np.ndim(scale) else float(scale), rng)
                    gi, ei = np.nonzero(hit)
                    if len(gi):
                        found = (c, int(mine[loud[ei[0]]]), g[gi[0]], None if old is None else old[gi[0]], f[loud[ei[0]]])
                        break
                if found is None:
                    raise AssertionError("window %d (%s): no %s witness in chunk class %d" % (w, windows[w], kind, cls))
                c, t, gain, old, value = found
                olds = None
                if old is not None:
                    olds = ((c, float(old)),)
                    if twin:
                        olds = ((0, float(old)), (1, _second_old(value, gain, old, rng)))
                out.append(VectorWitness(kind, w, c, t, np.float32(gain), olds))
    return out


def witness_histories():
    """the header samples of blocks 0 and 1 of the witness stream, in output order"""
    return [WITNESS_SAMPLES[:4], WITNESS_SAMPLES[4:]]
