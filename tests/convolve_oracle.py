"""The convolve stage (AADHip_Convolver*, include/aad_hip.h "reverberation") restated in numpy: the quantiser, the default delay,
the resolve, the exact 64-bit sums and the four element types (rows with a gain and a span: tests/window_placed_oracle.py over
to_float32).  The sums are formed by np.convolve over int64 - no byte planes, no tiles - so that nothing of the kernel's
arithmetic is shared with it.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import numpy as np

MAX_TAPS = 32768
MAX_TAP = 32639
NO_RESPONSE = 0xFFFFFFFF


def quantise(h, delay=None):
    """float32 taps -> (int16 taps, q, delay), None where the library refuses"""
    h = np.asarray(h, dtype=np.float32).reshape(-1)
    if not (1 <= h.size <= MAX_TAPS) or not np.all(np.isfinite(h)):
        return None
    if delay is not None and delay >= 0 and delay >= h.size:
        return None
    h64 = h.astype(np.float64)
    for q in range(15, -1, -1):
        hq = np.rint(h64 * float(1 << q))  # exact product, ties to even
        if np.max(np.abs(hq)) <= MAX_TAP:
            d = int(np.argmax(np.abs(hq))) if delay is None or delay < 0 else int(delay)  # argmax: the lowest index on ties
            return hq.astype(np.int16), q, d
    return None


def source_frames(frames, responses):
    return frames + max(len(r[0]) for r in responses) - 1


def resolve(stream, first_frame, response, responses):
    """-> (stream, src_first, lane response, shift); first_frame and response as unsigned 64-bit values"""
    first_frame &= (1 << 64) - 1
    response &= (1 << 64) - 1
    if response >= len(responses):
        return stream, first_frame, NO_RESPONSE, 0
    taps, _, d = responses[response]
    lead = len(taps) - 1 - d
    before = min(first_frame, lead)
    return stream, first_frame - before, response, before


def sums(x, first_frame, frames, taps, delay):
    """acc[n] = sum_k h[k] x[first_frame + n + delay - k], n < frames, x (a 1-d integer array) zero outside itself -> int64"""
    taps = np.asarray(taps, dtype=np.int64)
    K = len(taps)
    lo = first_frame + delay - (K - 1)  # the first frame the first output reads
    a, b = max(lo, 0), min(lo + frames + K - 1, len(x))  # the frames of x that the outputs read
    out = np.zeros(frames, dtype=np.int64)
    if b <= a:
        return out
    full = np.convolve(np.asarray(x[a:b], dtype=np.int64), taps)  # full[m] = sum_k taps[k] x[a + m - k]
    m = np.arange(frames) + first_frame + delay - a  # output n reads x[first_frame + n + delay - k]
    inside = (m >= 0) & (m < len(full))
    out[inside] = full[m[inside]]
    return out


def to_int16(acc, q):
    acc = np.asarray(acc, dtype=np.int64)
    v = (acc + (1 << (q - 1) if q else 0)) >> q  # an arithmetic shift: floor
    return np.clip(v, -32768, 32767).astype(np.int16)


def to_float32(acc, q):
    return np.asarray(acc, dtype=np.int64).astype(np.float32) * np.float32(2.0 ** -(15 + q))


def bf16_bits(f):
    """float32 -> the uint16 bits of bfloat16, rounded to nearest even (no NaN among the values here)"""
    u = np.asarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def element_bits(acc, q, kind):
    """the row elements as raw bits: kind in "int16", "float32", "float16", "bfloat16" """
    if kind == "int16":
        return to_int16(acc, q).view(np.uint16)
    f = to_float32(acc, q)
    if kind == "float32":
        return f.view(np.uint32)
    if kind == "float16":
        with np.errstate(over="ignore"):  # past 65504: inf, as the device rounds
            return f.astype(np.float16).view(np.uint16)
    return bf16_bits(f)


def row(x, stream_len, first_frame, frames, response):
    """acc of one window's channel row: x the stream's decode [>= stream_len] read as zero from stream_len on; response a
    (taps, q, delay) or None -> int64 [frames]"""
    if response is None:
        return np.zeros(frames, dtype=np.int64)
    first_frame &= (1 << 64) - 1
    if first_frame >= (1 << 62):  # huge and wrapped: nothing of the stream is read
        return np.zeros(frames, dtype=np.int64)
    taps, _, d = response
    return sums(np.asarray(x[:stream_len]), first_frame, frames, taps, d)
