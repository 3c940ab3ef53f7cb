"""The mix of the spectrogram stage (AADHip_SpectrogramRunMix, include/aad_hip.h "spectrogram", paragraph "mix") in numpy, written
from the definition's text: the staged sample x = clamp(rint(fl32(fl32(ga a) + fl32(gb b)))) - numpy rounds every float32
operation by itself, nothing fuses - over row buffers with pitches of their own, followed by spectrogram_oracle.spectrogram_rows
unchanged.  `mutant` names a mistake a kernel could make (MUTANTS); the GPU cases' inputs must tell each from the definition
(tests/test_spectrogram_mix_host.py).  `census` counts the witnesses those inputs must hold.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import numpy as np

import spectrogram_oracle as so

MUTANTS = ("fma", "ties_away", "truncate", "wrap", "nan_kept", "gain_by_row", "b_at_j", "span_end", "b_pitch_of_a")


def span_length(L, o, T):
    """Le: 0 for o >= T, else min(L, T - o); L, o: Python ints below 2^64"""
    L, o = int(L) & (2 ** 64 - 1), int(o) & (2 ** 64 - 1)
    return 0 if o >= T else min(L, T - o)


def quantise(m, mutant=None):
    """float32 array -> int16: a NaN 0, else the nearest integer, ties to even, clamped"""
    m = np.asarray(m, dtype=np.float32)
    nan = np.isnan(m)
    v = np.where(nan, np.float32(0), m).astype(np.float64)
    if mutant == "ties_away":
        r = np.sign(v) * np.floor(np.abs(v) + 0.5)
    elif mutant == "truncate":
        r = np.trunc(v)
    else:
        r = np.rint(v)  # ties to even
    if mutant == "wrap":
        finite = np.isfinite(r)
        low = (np.where(finite, r, 0).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)
        x = np.where(finite, low, np.where(r > 0, 32767, -32768)).astype(np.int16)
    else:
        x = np.clip(r, -32768, 32767).astype(np.int16)
    if mutant == "nan_kept":  # what a conversion that knows no NaN leaves: the most negative integer, clamped
        x = np.where(nan, np.int16(-32768), x)
    return x


def mix_element(ga, a, gb, b, inside, mutant=None):
    """the definition on arrays: ga, gb float32, a, b int16, inside bool -> int16"""
    ga, gb = np.asarray(ga, dtype=np.float32), np.asarray(gb, dtype=np.float32)
    af, bf = np.asarray(a, dtype=np.int16).astype(np.float32), np.asarray(b, dtype=np.int16).astype(np.float32)
    with np.errstate(all="ignore"):
        pa = ga * af  # float32, rounded
        if mutant == "fma":  # m + gb * b contracted: the product unrounded (exact in float64), one rounding of the sum
            both = (pa.astype(np.float64) + gb.astype(np.float64) * bf.astype(np.float64)).astype(np.float32)
        else:
            pb = gb * bf
            both = pa + pb
    return quantise(np.where(inside, both, pa), mutant)


def mix_buffers(buf_a, at_a, pitch_a, buf_b, at_b, pitch_b, R, T, rows_per_gain=1, gain_a=None, gain_b=None, spans=None, mutant=None):
    """x int16 [R, T]: row r of a at buf_a[at_a + r * pitch_a:], of b likewise; gains float32 [R / rows_per_gain] or None;
    spans: a list of (L, o) Python ints per group or None"""
    assert mutant is None or mutant in MUTANTS
    assert rows_per_gain >= 1 and R % rows_per_gain == 0
    groups = R // rows_per_gain
    x = np.zeros((R, T), dtype=np.int16)
    j = np.arange(T)
    for r in range(R):
        G = r % groups if mutant == "gain_by_row" else r // rows_per_gain
        ga = np.float32(1) if gain_a is None else np.float32(gain_a[G])
        gb = np.float32(1) if gain_b is None else np.float32(gain_b[G])
        L, o = (T, 0) if spans is None else spans[r // rows_per_gain]
        Le = span_length(L, o, T)
        o = int(o) if Le else 0
        end = o + Le - (1 if mutant == "span_end" and Le else 0)
        inside = (j >= o) & (j < end)
        a = buf_a[at_a + r * pitch_a: at_a + r * pitch_a + T]
        start_b = at_b + r * (pitch_a if mutant == "b_pitch_of_a" else pitch_b)
        b = np.zeros(T, dtype=np.int16)
        if mutant == "b_at_j":
            b[inside] = buf_b[start_b + j[inside]]
        else:
            b[inside] = buf_b[start_b + j[inside] - o]
        x[r] = mix_element(ga, a, gb, b, inside, mutant)
    return x


def mix_rows(a, b, rows_per_gain=1, gain_a=None, gain_b=None, spans=None, mutant=None):
    """contiguous int16 [R, T] rows"""
    a, b = np.ascontiguousarray(a, dtype=np.int16), np.ascontiguousarray(b, dtype=np.int16)
    R, T = a.shape
    return mix_buffers(a.reshape(-1), 0, T, b.reshape(-1), 0, T, R, T, rows_per_gain, gain_a, gain_b, spans, mutant)


def spectrogram_mix_rows(x, window, n_fft, H, filters=None):
    """the stage's output for a batch that holds x"""
    return so.spectrogram_rows(x, window, n_fft, H, filters)


def census(a, b, rows_per_gain, gain_a, gain_b, spans, boundary):
    """What contiguous rows witness: ties whose floor is even and odd, clamps at each rail, and the elements inside and outside
    b's span below and from element `boundary` of the row on -> dict of counts"""
    a, b = np.asarray(a, dtype=np.int16), np.asarray(b, dtype=np.int16)
    R, T = a.shape
    count = dict(tie_even_floor=0, tie_odd_floor=0, clamp_low=0, clamp_high=0, inside_before=0, inside_after=0, outside_before=0,
                 outside_after=0)
    j = np.arange(T)
    for r in range(R):
        G = r // rows_per_gain
        ga = np.float32(1) if gain_a is None else np.float32(gain_a[G])
        gb = np.float32(1) if gain_b is None else np.float32(gain_b[G])
        L, o = (T, 0) if spans is None else spans[G]
        Le = span_length(L, o, T)
        o = int(o) if Le else 0
        inside = (j >= o) & (j < o + Le)
        bs = np.zeros(T, dtype=np.int16)
        bs[inside] = b[r, j[inside] - o]
        with np.errstate(all="ignore"):
            pa = ga * a[r].astype(np.float32)
            m = np.where(inside, pa + gb * bs.astype(np.float32), pa).astype(np.float64)
        finite = np.isfinite(m)
        mf = np.where(finite, m, 0.0)
        tie = finite & (mf - np.floor(mf) == 0.5) & (np.abs(mf) < 32767)
        count["tie_even_floor"] += int((tie & (np.floor(mf) % 2 == 0)).sum())
        count["tie_odd_floor"] += int((tie & (np.floor(mf) % 2 == 1)).sum())
        count["clamp_low"] += int((m < -32768.5).sum())
        count["clamp_high"] += int((m > 32767.5).sum())
        count["inside_before"] += int((inside & (j < boundary)).sum())
        count["inside_after"] += int((inside & (j >= boundary)).sum())
        count["outside_before"] += int((~inside & (j < boundary)).sum())
        count["outside_after"] += int((~inside & (j >= boundary)).sum())
    return count
