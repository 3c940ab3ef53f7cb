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
windows that start on those blocks carry the witness gains.

TEST INFRASTRUCTURE (tests/ only)."""
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


def witness_histories():
    """the header samples of blocks 0 and 1 of the witness stream, in output order"""
    return [WITNESS_SAMPLES[:4], WITNESS_SAMPLES[4:]]
