"""The float16 / bfloat16 rows of window decode (include/aad_hip.h, AAD_HIP_SAMPLE_FLOAT16 and AAD_HIP_SAMPLE_BFLOAT16) restated
through torch on the CPU: the float32 row - the int16 sample * 2^-15, or the down-mix sum L + R * 2^-16, both exact - rounded once
by torch's own conversion.  tests/window_oracle.py and tests/channel_mix_oracle.py produce the int16 rows and the sums.

TEST INFRASTRUCTURE (tests/ only)."""
import numpy as np

HALF_DTYPES = ("float16", "bfloat16")


def torch_dtype(name):
    import torch
    return {"float16": torch.float16, "bfloat16": torch.bfloat16}[name]


def half_bits_of_float32(rows32, name):
    """float32 array -> uint16 array of the same shape: the bit patterns of rows32.to(dtype)"""
    import torch
    rows32 = np.ascontiguousarray(rows32, dtype=np.float32)
    t = torch.from_numpy(rows32).to(torch_dtype(name))
    return t.view(torch.int16).numpy().view(np.uint16).reshape(rows32.shape)


def half_bits_expected(rows16, name, scale=32768.0):
    """int array (int16 rows; with scale = 65536 the down-mix sums L + R) -> uint16 bit patterns of the dtype's rows"""
    rows = np.asarray(rows16)
    assert rows.dtype.kind == "i" and np.abs(rows.astype(np.int64)).max(initial=0) <= scale
    return half_bits_of_float32(rows.astype(np.float32) / np.float32(scale), name)


def bfloat16_bits_by_integer_rounding(rows32):
    """float32 array -> uint16: round to nearest even on the float32 bits, in integers (finite values that do not overflow)"""
    u = np.ascontiguousarray(rows32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
