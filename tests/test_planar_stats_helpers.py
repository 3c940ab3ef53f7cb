"""aad_amd.engine.rmse / snr_db / select_least_bits (the selection Engine.least_bits makes) on hand-made CPU tensors: the
definitions, an empty row (count == 0 -> NaN), a zero error (+inf), and sums above 2^53, which must go int64 -> float64 and never
through float32."""
import math

import pytest

torch = pytest.importorskip("torch")

from aad_amd.engine import rmse, select_least_bits, snr_db  # noqa: E402


def rec(sum_sq, sum_abs, max_abs, count):
    return [sum_sq, sum_abs, max_abs, count]


def test_rmse_definition_empty_row_and_large_sums():
    big = 65535 ** 2 * (2 ** 31 - 1)  # the largest sum of squares of a row below 2^31 frames: > 2^62
    stats = torch.tensor([[rec(400, 40, 7, 4), rec(0, 0, 0, 16)],
                          [rec(0, 0, 0, 0), rec(big, 65535 * (2 ** 31 - 1), 65535, 2 ** 31 - 1)]], dtype=torch.int64)
    got = rmse(stats)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 2)
    assert got[0, 0].item() == 10.0 and got[0, 1].item() == 0.0
    assert math.isnan(got[1, 0].item())
    assert got[1, 1].item() == 65535.0


def test_conversion_never_passes_through_float32():
    # 2^53 + 2^30 and 2^53 differ by 2^30: float64 keeps that, float32 (24-bit mantissa) rounds both to 2^53
    a, b = 2 ** 53 + 2 ** 30, 2 ** 53
    stats = torch.tensor([rec(a, 0, 0, 2 ** 20), rec(b, 0, 0, 2 ** 20)], dtype=torch.int64)
    r = rmse(stats)
    # the division is exact (a power of two); torch's vectorised sqrt / log10 may round the last bit unlike libm's: 2 ulp of float64
    ulp2 = 2 * 2.0 ** -52
    assert r[0].item() == pytest.approx(math.sqrt(float(a) / 2 ** 20), rel=ulp2, abs=0)
    assert r[1].item() == pytest.approx(math.sqrt(float(b) / 2 ** 20), rel=ulp2, abs=0)
    assert r[0].item() > r[1].item()  # through float32 the two would be equal
    s = snr_db(stats, torch.tensor([a, a], dtype=torch.int64))
    want = 10.0 * math.log10(float(a) / float(b))  # 5.2e-7 dB: the quotient is 1 + 2^-23 exactly, so the bound below is on log10 alone
    assert s[0].item() == 0.0 and s[1].item() > 0.0 and s[1].item() == pytest.approx(want, rel=1e-9, abs=0)
    # the signal power may come as int64 above 2^53 too, or as a float tensor
    s2 = snr_db(stats, torch.tensor([float(a), float(a)], dtype=torch.float64))
    assert torch.equal(s, s2)


def test_snr_db_definition_zero_error_and_empty_row():
    stats = torch.tensor([rec(100, 10, 5, 50), rec(0, 0, 0, 50), rec(0, 0, 0, 0), rec(1000, 0, 0, 10)], dtype=torch.int64)
    got = snr_db(stats, torch.tensor([100000, 12345, 0, 0], dtype=torch.int64))
    assert got.dtype == torch.float64
    assert got[0].item() == pytest.approx(30.0, abs=1e-12)
    assert got[1].item() == math.inf                      # no error at all, whatever the signal
    assert math.isnan(got[2].item())                      # an empty row
    assert got[3].item() == -math.inf                     # silence in, noise out
    assert snr_db(torch.tensor(rec(0, 0, 0, 9)), 0).item() == math.inf  # silence coded exactly, a Python scalar as signal
    with pytest.raises(ValueError):
        rmse(stats.to(torch.int32))
    with pytest.raises(ValueError):
        snr_db(stats[:, :3], 1)


def test_least_bits_selection():
    inf, nan = math.inf, math.nan
    #            stream: 0 all pass   1 only 4   2 none      3 one channel holds it back   4 exact   5 empty row   6 at the bound
    snr2 = torch.tensor([[40.0, 41], [10, 50], [1, 2], [35, 12], [inf, inf], [nan, 50], [30.0, 30.0]], dtype=torch.float64)
    snr3 = torch.tensor([[50.0, 51], [20, 60], [5, 6], [45, 31], [inf, inf], [nan, 60], [10.0, 10.0]], dtype=torch.float64)
    snr4 = torch.tensor([[60.0, 61], [30, 70], [9, 29.999], [55, 40], [inf, inf], [nan, 70], [10.0, 10.0]], dtype=torch.float64)
    got = select_least_bits([snr2, snr3, snr4], 30.0)
    assert got.dtype == torch.int64
    assert got.tolist() == [2, 4, 0, 3, 2, 0, 2]
    assert select_least_bits([snr2, snr3, snr4], 100.0).tolist() == [0, 0, 0, 0, 2, 0, 0]
    assert select_least_bits([snr2, snr3, snr4], -inf).tolist() == [2, 2, 2, 2, 2, 0, 2]
