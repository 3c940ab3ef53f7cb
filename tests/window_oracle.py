"""The window decode's definition (include/aad_hip.h, "window decode") restated in numpy: slice the whole-stream decode, pad with
zeros, convert.  D_s is what AADHip_DecodePlanRun writes for stream s into a zero-filled buffer of num_samples frames; for images
an encoder wrote that is the oracle's decode (tests/oracle_binding.py).

TEST INFRASTRUCTURE (tests/ only)."""
import numpy as np

U64 = 1 << 64


def window_expected(decoded, windows, frames, channels, dtype=np.int16):
    """decoded: list of int16 arrays [num_samples, channels] (D_s per stream of the plan); windows: int array [N, 2] of
    (stream, first_frame), read as uint64 (negative int64 values wrap); -> [N, channels, frames] of int16, or float32 = int16 / 32768"""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((len(windows), channels, frames), dtype=np.int16)
    for w, (s, f) in enumerate(windows.tolist()):
        s, f = s % U64, f % U64
        if s >= len(decoded):
            continue
        d = decoded[s]
        if f >= d.shape[0]:
            continue
        part = d[f:f + frames]
        out[w, :, :part.shape[0]] = part.T
    if dtype == np.float32:
        return out.astype(np.float32) / np.float32(32768.0)
    return out
