"""The spectrogram stage's definition (include/aad_hip.h "spectrogram") in numpy, written from the definition's text: the
quantised cos / -sin matrices, the frame count, the exact integer sums, the float32 elements one operation at a time - numpy
rounds every float32 operation by itself, nothing fuses - and the filterbank sum in ascending order.  `mutant` names a mistake a
kernel could make (MUTANTS); the GPU cases must tell each from the definition.  Also mel_filters' formula restated, and a float64
STFT for the accuracy table (tools/spectrogram_probe.py --accuracy)."""
import numpy as np

MAX_COEFFICIENT = 32639

MUTANTS = ("no_constant", "stride_w", "late", "fma", "exact_square", "descending", "neighbour_tile", "first_span")


def hann(win_length):
    """the periodic Hann window, in float64, rounded to float32"""
    n = np.arange(win_length, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)).astype(np.float32)


def bins(n_fft):
    return n_fft // 2 + 1


def quantise(window, n_fft):
    """-> (q, cq, sq): int16 [W, B] each; None when q = 0 does not fit"""
    window = np.asarray(window, dtype=np.float32)
    W, B = window.size, bins(n_fft)
    assert 1 <= W <= n_fft <= 4096 and np.isfinite(window).all()
    m = (np.arange(W, dtype=np.int64)[:, None] * np.arange(B, dtype=np.int64)[None, :]) % n_fft
    angle = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
    w = window.astype(np.float64)[:, None]
    c = w * np.cos(angle)[m]
    s = -w * np.sin(angle)[m]
    for q in range(15, -1, -1):
        cq, sq = np.rint(np.ldexp(c, q)), np.rint(np.ldexp(s, q))
        if max(np.abs(cq).max(), np.abs(sq).max()) <= MAX_COEFFICIENT:
            return q, cq.astype(np.int16), sq.astype(np.int16)
    return None


def frames(T, W, H):
    """F, None for T < W"""
    return None if T < W else 1 + (T - W) // H


def frame_matrix(x, W, H, F, offset=0, stride=None):
    """int64 [F, W]: row f is x[f * stride + offset + t], zero past the row's end"""
    stride = H if stride is None else stride
    x = np.asarray(x, dtype=np.int64)
    padded = np.concatenate([x, np.zeros(max(0, (F - 1) * stride + offset + W - x.size), dtype=np.int64)])
    at = np.arange(F, dtype=np.int64)[:, None] * stride + offset + np.arange(W, dtype=np.int64)[None, :]
    return padded[at]


def sums(x, cq, sq, H, offset=0, stride=None):
    """the exact Re, Im: int64 [F, B].  Every partial sum is an integer below 2^42, so the float64 products are exact."""
    W = cq.shape[0]
    F = frames(len(x), W, H)
    X = frame_matrix(x, W, H, F, offset, stride).astype(np.float64)
    return (X @ cq.astype(np.float64)).astype(np.int64), (X @ sq.astype(np.float64)).astype(np.int64)


def element(S, q):
    """fl32(S) 2^-(15 + q): one rounding of the 64-bit integer, then an exact scale"""
    return np.asarray(S, dtype=np.int64).astype(np.float32) * np.float32(2.0 ** -(15 + q))


def power(Re, Im, q):
    re, im = element(Re, q), element(Im, q)
    a = re * re  # float32, rounded
    b = im * im
    return a + b


def bands(filters):
    """[(lo, hi)] per filter; an all-zero one is (B, 0)"""
    out = []
    for row in np.asarray(filters, dtype=np.float32):
        nz = np.flatnonzero(row)
        out.append((int(nz[0]), int(nz[-1])) if nz.size else (row.size, 0))
    return out


def filterbank(P, filters, descending=False):
    """E[f][j]: from +0, E = fl32(E + fl32(w[j][k] P[f][k])) for k = lo .. hi in that order"""
    filters = np.asarray(filters, dtype=np.float32)
    E = np.zeros((P.shape[0], filters.shape[0]), dtype=np.float32)
    for j, (lo, hi) in enumerate(bands(filters)):
        order = range(lo, hi + 1)
        for k in (reversed(order) if descending else order):
            E[:, j] = E[:, j] + filters[j, k] * P[:, k]
    return E


def spectrogram(x, window, n_fft, H, filters=None, mutant=None, tile_frames=256):
    """One row x (int16 [T]) -> float32 [F, M], or [F, B] without filters.  mutant: one of MUTANTS, None for the definition."""
    assert mutant is None or mutant in MUTANTS
    q, cq, sq = quantise(window, n_fft)
    W, B = cq.shape
    x = np.asarray(x, dtype=np.int16)
    F = frames(x.size, W, H)
    Re, Im = sums(x, cq, sq, H, offset=1 if mutant == "late" else 0, stride=W if mutant == "stride_w" else None)
    if mutant == "no_constant":  # the low bytes' offset of 128 left in: every sample 128 lower
        Re = Re - 128 * cq.astype(np.int64).sum(0)
        Im = Im - 128 * sq.astype(np.int64).sum(0)
    if mutant == "first_span" and F > tile_frames:
        Re[tile_frames:], Im[tile_frames:] = Re[:F - tile_frames].copy(), Im[:F - tile_frames].copy()
    if mutant == "fma":
        re, im = element(Re, q).astype(np.float64), element(Im, q).astype(np.float64)
        P = (re * re + (im * im).astype(np.float32).astype(np.float64)).astype(np.float32)
    elif mutant == "exact_square":
        exact = [[int(a) * int(a) + int(b) * int(b) for a, b in zip(ra, rb)] for ra, rb in zip(Re.tolist(), Im.tolist())]
        P = np.array([[np.float32(v / 4.0 ** (15 + q)) if v < 2 ** 1000 else 0 for v in row] for row in exact], dtype=np.float32).reshape(F, B)
    else:
        P = power(Re, Im, q)
    if mutant == "neighbour_tile" and B % 16 != 0 and B > 16:
        first = B // 16 * 16
        P = P.copy()
        P[:, first:] = P[:, first - 16:first - 16 + (B - first)]
    if filters is None:
        return P
    return filterbank(P, filters, descending=mutant == "descending")


def spectrogram_rows(rows, window, n_fft, H, filters=None, mutant=None, tile_frames=256):
    """rows int16 [..., T] -> [..., F, columns]"""
    rows = np.asarray(rows, dtype=np.int16)
    flat = rows.reshape(-1, rows.shape[-1])
    out = np.stack([spectrogram(r, window, n_fft, H, filters, mutant, tile_frames) for r in flat])
    return out.reshape(rows.shape[:-1] + out.shape[1:])


# ---- mel_filters' formula, restated ------------------------------------------------------------------------------------------------

def mel_filters(rate, n_fft, n_mels, f_min=0.0, f_max=None):
    """HTK triangles, unnormalised, element by element in Python floats (float64) -> float32 [n_mels, B]"""
    import math
    f_max = rate / 2.0 if f_max is None else f_max
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    lo, hi = mel(f_min), mel(f_max)
    points = [700.0 * (10.0 ** (m / 2595.0) - 1.0) for m in np.linspace(lo, hi, n_mels + 2).tolist()]
    out = np.zeros((n_mels, bins(n_fft)), dtype=np.float32)
    for j in range(n_mels):
        for k in range(bins(n_fft)):
            f = k * float(rate) / n_fft
            w = max(0.0, min((f - points[j]) / (points[j + 1] - points[j]), (points[j + 2] - f) / (points[j + 2] - points[j + 1])))
            w = np.float32(w)
            out[j, k] = w if abs(w) >= 2.0 ** -60 else 0
    return out


def frame_counts(count, W, H):
    """the frames that lie wholly inside the first `count` elements, by counting"""
    return sum(1 for f in range(count) if f * H + W <= count) if count >= W else 0


# ---- the float64 reference of the accuracy table -------------------------------------------------------------------------------------

def reference_float64(x, window, n_fft, H, filters=None):
    """a float64 STFT of the waveform x / 32768 with the float32 window widened, abs() ** 2, and the filters in float64"""
    W = len(window)
    F = frames(len(x), W, H)
    X = frame_matrix(x, W, H, F).astype(np.float64) / 32768.0 * np.asarray(window, dtype=np.float64)[None, :]
    P = np.abs(np.fft.rfft(X, n=n_fft, axis=1)) ** 2
    return P if filters is None else P @ np.asarray(filters, dtype=np.float64).T
