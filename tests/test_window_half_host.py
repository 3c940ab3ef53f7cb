"""The float16 / bfloat16 sample types of window decode, on the host: the oracle function of the GPU tests
(tests/window_half_oracle.py) pinned against the hand values of include/aad_hip.h's definition and against an integer
round-to-nearest-even of the float32 bits, and the numbers of the two sample types in the header and in aad_amd.capi."""
import os
import re

import numpy as np
import pytest

from window_half_oracle import bfloat16_bits_by_integer_rounding, half_bits_expected, half_bits_of_float32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_INT16 = np.arange(-32768, 32768, dtype=np.int32)
ALL_SUMS = np.arange(-65536, 65535, dtype=np.int32)  # L + R of two int16


def _bits(values, name, scale=32768.0):
    return half_bits_expected(np.asarray(values, dtype=np.int32), name, scale).tolist()


def _back(bits, name):
    """uint16 bit patterns -> the float32 values they stand for"""
    bits = np.asarray(bits, dtype=np.uint16)
    if name == "bfloat16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def test_sample_type_numbers():
    from aad_amd import capi
    assert (capi.SAMPLE_INT16, capi.SAMPLE_FLOAT32, capi.SAMPLE_FLOAT16, capi.SAMPLE_BFLOAT16) == (0, 1, 4, 5)
    with open(os.path.join(ROOT, "include", "aad_hip.h")) as f:
        text = f.read()
    body = re.search(r"enum AADHipSampleType \{(.*?)\};", text, re.S).group(1)
    declared = {m.group(1): int(m.group(2)) for m in re.finditer(r"AAD_HIP_SAMPLE_(\w+) = (-?\d+)", body)}
    assert declared == {"INT16": 0, "FLOAT32": 1, "FLOAT16": 4, "BFLOAT16": 5}


def test_smallest_values_are_subnormals_and_not_zero():
    assert _bits([1, -1], "float16") == [0x0200, 0x8200]
    assert _bits([1, -1], "float16", 65536.0) == [0x0100, 0x8100]  # the smallest down-mix sum, 2^-16
    assert _bits([0], "float16") == [0] and _bits([0], "bfloat16") == [0]
    for name in ("float16", "bfloat16"):
        for values, scale in ((ALL_INT16, 32768.0), (ALL_SUMS, 65536.0)):
            bits = half_bits_expected(values, name, scale)
            assert ((bits & 0x7FFF) != 0).sum() == len(values) - 1  # no non-zero value rounds to zero
            assert bits[values == 0].tolist() == [0]              # and zero is +0


def test_ties_go_to_even():
    assert _bits([2049, 2051, -2049, -2051], "float16") == _bits([2048, 2052, -2048, -2052], "float16")
    assert _bits([257, 259, -257, -259], "bfloat16") == _bits([256, 260, -256, -260], "bfloat16")
    # every odd |sample| of the binade is a tie, and none resolves to an odd neighbour's pattern
    for name, lo, step in (("float16", 2048, 2), ("bfloat16", 256, 2)):
        odd = np.arange(lo + 1, 2 * lo, 2, dtype=np.int32)
        got = _back(half_bits_expected(odd, name), name) * 32768.0
        assert (np.abs(got - odd) == 1).all() and (got % (2 * step) == 0).all()


def test_rails():
    assert _bits([32767], "float16") == [0x3C00] and _bits([32767], "bfloat16") == [0x3F80]  # +1.0
    assert _bits([-32768, -32767], "float16") == [0xBC00, 0xBC00]                          # -1.0, both
    assert _bits([-32768], "bfloat16") == [0xBF80]
    assert _bits([-65536, 65534], "float16", 65536.0) == [0xBC00, 0x3C00]                  # the corners of the down-mix


@pytest.mark.parametrize("name,exact", [("float16", 12288), ("bfloat16", 2304)])
def test_exact_value_counts_over_all_int16(name, exact):
    want = ALL_INT16.astype(np.float32) / np.float32(32768.0)
    got = _back(half_bits_expected(ALL_INT16, name), name)
    assert int((got == want).sum()) == exact
    ulp = 2.0 ** -10 if name == "float16" else 2.0 ** -7
    assert (np.abs(got - want) <= np.abs(want) * ulp / 2).all()  # a nearest rounding: within half a unit of the last place


def test_bfloat16_is_integer_round_to_nearest_even_of_the_float32_bits():
    for values, scale in ((ALL_INT16, 32768.0), (ALL_SUMS, 65536.0)):
        rows32 = values.astype(np.float32) / np.float32(scale)
        assert np.array_equal(half_bits_of_float32(rows32, "bfloat16"), bfloat16_bits_by_integer_rounding(rows32))


def test_float16_is_numpys_conversion_of_the_float32_value():
    for values, scale in ((ALL_INT16, 32768.0), (ALL_SUMS, 65536.0)):
        rows32 = values.astype(np.float32) / np.float32(scale)
        assert np.array_equal(half_bits_of_float32(rows32, "float16"), rows32.astype(np.float16).view(np.uint16))


def test_down_mix_corners():
    """odd L + R keeps its half step through the float32 value into the float16 row"""
    sums = np.array([-65536, 65534, -3, -1, 1, 4097], dtype=np.int32)
    f16 = half_bits_expected(sums, "float16", 65536.0)
    assert f16.tolist() == [0xBC00, 0x3C00, 0x8300, 0x8100, 0x0100] + [int(np.float16(4097 / 65536.0).view(np.uint16))]
    assert f16[2] != half_bits_expected(np.array([-2], dtype=np.int32), "float16")[0]  # not the floor mix's row
