"""The resample stage's definition (include/aad_hip.h, "resample") restated in numpy, all in integers but for the bank's
construction, which is double precision here as in the library: the reduction, the bank, the source batch's length, the resolve
and a row's FIR and conversion.  The int16 rows it is fed come from tests/window_oracle.py (the whole decode of each stream).

TEST INFRASTRUCTURE (tests/ only)."""
from math import gcd

import numpy as np

from window_half_oracle import half_bits_of_float32

U64 = 1 << 64
UNITY = 16384
NO_BANK = 0xFFFF


def reduce_ratio(up, down):
    g = gcd(up, down)
    return up // g, down // g


def taps(L, M):
    """K: 2 for the identity, else 2 * ceil(12 / s), s = min(1, L / M)"""
    if (L, M) == (1, 1):
        return 2
    return 24 if L >= M else 2 * -(-12 * M // L)


def prototype(t, L, M, K):
    """g(t), double precision"""
    s = min(1.0, L / M)
    t = np.asarray(t, dtype=np.float64)
    inside = np.abs(t) <= K / 2
    u = np.where(inside, 1 - (t / (K / 2)) ** 2, 0.0)
    g = 0.94 * s * np.sinc(0.94 * s * t) * np.i0(9 * np.sqrt(np.maximum(u, 0.0))) / np.i0(9.0)
    return np.where(inside, g, 0.0)


def bank(L, M):
    """int64 [L, K]: scale each phase to 16384, floor, 1 more to the taps with the largest fractional parts (ties to the lower k)"""
    K = taps(L, M)
    if (L, M) == (1, 1):
        return np.array([[UNITY, 0]], dtype=np.int64)
    h = np.zeros((L, K), dtype=np.int64)
    k = np.arange(K)
    for p in range(L):
        g = prototype(k - (K // 2 - 1) - p / L, L, M, K)
        v = g * UNITY / g.sum()
        fl = np.floor(v)
        rest = UNITY - int(fl.sum())
        order = np.argsort(-(v - fl), kind="stable")  # stable: equal fractional parts keep the lower k first
        fl[order[:rest]] += 1
        h[p] = fl.astype(np.int64)
    return h


def limits_ok(up, down):
    """what AADHip_ResamplerCreate accepts of a ratio, but for the sum |h| rule (which needs the bank)"""
    if up == 0 or down == 0:
        return False
    L, M = reduce_ratio(up, down)
    K = taps(L, M)
    return L <= 1024 and K <= 256 and 2 * L * K <= 65536


def source_frames(frames, banks):
    """T_src over (L, M, K) triples"""
    return max((frames - 1) * M // L + K for L, M, K in banks)


def resolve(first_frame, K):
    """-> (src_first, shift)"""
    first_frame %= U64
    shift = min(first_frame, K // 2 - 1)
    return first_frame - shift, shift


def fir(x, first_frame, frames, L, M, h):
    """x: int array, one channel of a stream's whole decode; -> int64 acc[frames]: zero before frame 0 and from len(x) on"""
    h = np.asarray(h, dtype=np.int64)
    K = h.shape[1]
    first_frame %= U64
    n = np.arange(frames, dtype=np.int64)
    i, p = n * M // L, n * M % L
    acc = np.zeros(frames, dtype=np.int64)
    if first_frame - (K // 2 - 1) >= len(x):  # nothing of the stream under any tap
        return acc
    x = np.asarray(x, dtype=np.int64)
    at = first_frame + i[:, None] + np.arange(K)[None, :] - (K // 2 - 1)  # [frames, K]
    inside = (at >= 0) & (at < len(x))
    acc = (h[p] * np.where(inside, x[np.clip(at, 0, max(len(x) - 1, 0))] if len(x) else 0, 0)).sum(axis=1)
    assert np.abs(acc).max(initial=0) < 1 << 31
    return acc


def convert(acc, dtype):
    """acc: int64 array -> int16, or the bit patterns of the float types (uint32 for float32, uint16 for the 2-byte ones)"""
    acc = np.asarray(acc, dtype=np.int64)
    if dtype == "int16":
        return np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16)  # >> floors
    f32 = acc.astype(np.float32) * np.float32(2.0 ** -29)  # int64 -> float32: one rounding to nearest even; the scale is exact
    if dtype == "float32":
        return f32.view(np.uint32)
    return half_bits_of_float32(f32, dtype)


def expected_acc(decoded, windows, variant, select, banks, frames, channels):
    """decoded: per stream an int16 array [num_samples, channels] (the rows a window decode plan writes, tests/window_oracle.py's
    input); windows: [N, 2]; variant: [N] or None; select: [num_streams][V] of bank indices or NO_BANK; banks: list of (L, M, h)
    -> int64 acc [N, channels, frames], zeros for a window without a bank; convert() gives the rows of a sample type"""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    select = np.asarray(select).reshape(len(select), -1)
    out = np.zeros((len(windows), channels, frames), dtype=np.int64)
    for w, (s, f) in enumerate(windows.tolist()):
        v = 0 if variant is None else int(variant[w]) % U64
        s %= U64
        if s >= select.shape[0] or v >= select.shape[1] or select[s][v] == NO_BANK:
            continue
        L, M, h = banks[int(select[s][v])]
        for c in range(channels):
            x = decoded[s][:, c] if s < len(decoded) else np.zeros(0, dtype=np.int16)
            out[w, c] = fir(x, f, frames, L, M, h)
    return out


def expected(decoded, windows, variant, select, banks, frames, channels, dtype):
    return convert(expected_acc(decoded, windows, variant, select, banks, frames, channels), dtype)
