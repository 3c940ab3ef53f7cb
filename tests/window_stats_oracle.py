"""The window decode statistics' definition (include/aad_hip.h, AADHip_WindowDecodePlanRunStats) restated in numpy over the int16
expectation of the window decode itself (tests/window_oracle.py, tests/channel_mix_oracle.py): per row (w, r) of the [N, C, T]
int16 rows v

  sum_sq = sum v^2,  sum_abs = sum |v|,  max_abs = max |v| (0 for an empty row),
  count  = min(T, num_samples[stream] - first_frame), 0 for a stray window, a wrapped value and first_frame >= num_samples

as an int64 [N, C, 4] table.  The sums are taken in int64 (python ints for the check of that), count from the lengths alone: a
truncated image changes the rows, never the count.

TEST INFRASTRUCTURE (tests/ only)."""
import numpy as np

from channel_mix_oracle import channel_mix_expected
from window_oracle import window_expected

U64 = 1 << 64


def window_counts(lengths, windows, frames):
    """int64 [N]: the frames of each window its stream has, from the table's lengths alone"""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(windows), dtype=np.int64)
    for w, (s, f) in enumerate(windows.tolist()):
        s, f = s % U64, f % U64
        if s < len(lengths) and f < int(lengths[s]):
            out[w] = min(int(frames), int(lengths[s]) - f)
    return out


def stats_of_rows(rows, counts):
    """rows: int16 [N, C, T]; counts: int64 [N] -> int64 [N, C, 4] of (sum_sq, sum_abs, max_abs, count)"""
    rows = np.asarray(rows)
    assert rows.dtype == np.int16 and rows.ndim == 3
    wide = np.abs(rows.astype(np.int64))  # |-32768| = 32768
    out = np.zeros(rows.shape[:2] + (4,), dtype=np.int64)
    out[..., 0] = (wide * wide).sum(axis=-1)
    out[..., 1] = wide.sum(axis=-1)
    out[..., 2] = wide.max(axis=-1, initial=0)
    out[..., 3] = np.asarray(counts, dtype=np.int64)[:, None]
    return out


def window_stats_expected(decoded, windows, frames, channels, lengths=None):
    """decoded: list of int16 [num_samples, channels] (D_s of window_oracle); lengths: the table's num_samples, default those of
    `decoded` -> int64 [N, channels, 4]"""
    lengths = [d.shape[0] for d in decoded] if lengths is None else lengths
    return stats_of_rows(window_expected(decoded, windows, frames, channels, np.int16), window_counts(lengths, windows, frames))


def channel_mix_stats_expected(decoded, windows, frames, out_channels, lengths=None):
    """decoded: list of int16 [num_samples, C_s], C_s 1 or 2 -> int64 [N, out_channels, 4]: the statistics of the INT16 mix, whatever
    sample type a run writes"""
    lengths = [d.shape[0] for d in decoded] if lengths is None else lengths
    return stats_of_rows(channel_mix_expected(decoded, windows, frames, out_channels, np.int16),
                         window_counts(lengths, windows, frames))
