"""Window decode with a span per window (include/aad_hip.h, AADHip_WindowDecodePlanRunPlaced / ...RunPlacedStats) restated through
torch on the CPU, on top of tests/window_oracle.py / tests/channel_mix_oracle.py (the float32 and int16 rows of the whole crop)
and tests/window_gain_oracle.py (the multiply, the add and the one rounding of the type).  Per window, with (L, o) its span:

    Le  = 0 if o >= T else min(L, T - o)                     L, o read as uint64
    row = zeros (STORE) or out[w] (ADD)
    row[:, o:o+Le] = (row[:, o:o+Le].float() + g * row_float32[:, :Le]).to(dtype)       without `row.float() +` under STORE

and the statistics are those of the first Le frames of the int16 rows, count = min(Le, num_samples - first_frame).

TEST INFRASTRUCTURE (tests/ only)."""
import numpy as np

import window_gain_oracle as go
from window_stats_oracle import stats_of_rows, window_counts

U64 = 1 << 64


def span_frames(num_frames, out_frame, frames):
    """Le of one span; python ints, negative int64 values wrap"""
    num_frames, out_frame = int(num_frames) % U64, int(out_frame) % U64
    if out_frame >= frames:
        return 0
    return min(num_frames, frames - out_frame)


def clipped(spans, n, frames):
    """spans: int array [N, 2] or None (every span is (T, 0)) -> list of (Le, o); o is 0 where Le is 0"""
    if spans is None:
        return [(frames, 0)] * n
    pairs = spans.reshape(-1, 2).tolist() if isinstance(spans, np.ndarray) else [tuple(p) for p in spans]  # python ints: no float detour
    assert len(pairs) == n
    out = []
    for length, o in pairs:
        le = span_frames(length, o, frames)
        out.append((le, int(o) % U64 if le else 0))
    return out


def placed_expected(rows32, spans, gain, name, old_bits=None):
    """rows32: float32 [N, C, T], the rows of the run without spans; spans: int [N, 2] of (num_frames, out_frame) or None;
    gain: float32 [N] or None; old_bits: None - STORE - or the bit patterns the rows held - ADD -> the rows' bit patterns"""
    rows32 = np.ascontiguousarray(rows32, dtype=np.float32)
    n, _, frames = rows32.shape
    out = np.zeros(rows32.shape, dtype=np.uint32 if name == "float32" else np.uint16) if old_bits is None else np.array(old_bits)
    gains = np.ones(n, dtype=np.float32) if gain is None else np.asarray(gain, dtype=np.float32)
    for w, (le, o) in enumerate(clipped(spans, n, frames)):
        if le:
            old = None if old_bits is None else out[w:w + 1, :, o:o + le]
            out[w:w + 1, :, o:o + le] = go.gain_expected(rows32[w:w + 1, :, :le], gains[w:w + 1], name, old)
    return out


def placed_stats_expected(rows16, lengths, windows, spans):
    """rows16: int16 [N, C, T], the int16 rows of the run without spans (a down-mix: the floor mix); lengths: the table's
    num_samples -> int64 [N, C, 4] of (sum_sq, sum_abs, max_abs, count) over each window's first Le frames"""
    rows16 = np.array(rows16)
    assert rows16.dtype == np.int16
    n, _, frames = rows16.shape
    counts = window_counts(lengths, windows, frames)
    for w, (le, _) in enumerate(clipped(spans, n, frames)):
        rows16[w, :, le:] = 0
        counts[w] = min(le, int(counts[w]))
    return stats_of_rows(rows16, counts)
