"""The channel-mix window decode's definition (include/aad_hip.h, AADHip_ChannelMixWindowDecodePlanCreate) restated in numpy: mix
each stream's whole decode D_s [num_samples, C_s] (C_s 1 or 2) to the output's channel count, then slice and pad with zeros as
tests/window_oracle.py does.

  C_s == C:           int16 the sample, float32 the sample / 32768
  C_s == 1, C == 2:   the one channel in both rows
  C_s == 2, C == 1:   int16 (L + R) >> 1 (floor); float32 (L + R) / 65536, exact - NOT the int16 mix / 32768

TEST INFRASTRUCTURE (tests/ only)."""
import numpy as np

U64 = 1 << 64


def mix_stream(d, out_channels, dtype=np.int16):
    """d: int16 [num_samples, C_s] -> [num_samples, out_channels] of int16 or float32"""
    d = np.asarray(d)
    assert d.dtype == np.int16 and d.ndim == 2 and d.shape[1] in (1, 2) and out_channels in (1, 2)
    wide = d.astype(np.int32)
    if d.shape[1] == out_channels:
        scale = 32768.0
    elif d.shape[1] == 1:
        wide, scale = np.repeat(wide, 2, axis=1), 32768.0
    else:
        wide, scale = wide[:, :1] + wide[:, 1:], 65536.0          # L + R: 17 bits, exact in float32
        if dtype == np.int16:
            wide = wide >> 1                                       # arithmetic: the floor of the mean
    if dtype == np.int16:
        assert wide.min(initial=0) >= -32768 and wide.max(initial=0) <= 32767
        return wide.astype(np.int16)
    assert dtype == np.float32
    return wide.astype(np.float32) / np.float32(scale)


def channel_mix_expected(decoded, windows, frames, out_channels, dtype=np.int16):
    """decoded: list of int16 arrays [num_samples, C_s]; windows: int array [N, 2] of (stream, first_frame), read as uint64 ->
    [N, out_channels, frames] of dtype"""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    mixed = {}
    out = np.zeros((len(windows), out_channels, frames), dtype=dtype)
    for w, (s, f) in enumerate(windows.tolist()):
        s, f = s % U64, f % U64
        if s >= len(decoded) or f >= decoded[s].shape[0]:
            continue
        if s not in mixed:
            mixed[s] = mix_stream(decoded[s], out_channels, dtype)
        part = mixed[s][f:f + frames]
        out[w, :, :part.shape[0]] = part.T
    return out
