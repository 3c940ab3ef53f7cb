"""The tie rule of the reconstruction statistics (aad_amd/csrc/aad_compare_round.h), proven on the CPU with exact arithmetic.

compare_finish_kernel sums a stream's e^2 and |e| in a fixed tree and prints, through `aad -c`, six decimals of
RMSE = sqrt(sum e^2 / n) and MSD = sum |e| / n.  The reference sums the same values in another order.  The kernel re-sums in
the reference's order when compare_crosses_boundary(v, compare_reorder_bound(n)) says that a %f rounding boundary
(k + 1/2) 1e-6 lies close enough to its value v for the order to show.  This test builds tests/compare_round_driver.cpp with
g++ against the header and checks that rule against the bound delta(n) derived here (u = 2^-53):

  * Any order of summing n non-negative terms lands within gamma of the exact sum, gamma_k = k u / (1 - k u) (Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2).  The reference's terms are fl(e^2) and it adds them in n - 1
    roundings; the device may contract e * e + s into one fused multiply-add, so its terms are the exact squares and it
    rounds n times.  Both lie within gamma_n of sum e^2 (exact squares), so the ratio of the two sums is at most
    A = (1 + gamma_n) / (1 - gamma_n).  Sum |e| has exact terms and the same bound.
  * Each side divides by n with one correctly rounded division: D = (1 + u) / (1 - u) more.  MSD: A D.
  * RMSE takes a correctly rounded square root of that quotient: sqrt(A D) D, bounded above by (1 + A D) / 2 D.
  * delta(n) = max(A D, (1 + A D) / 2 D) - 1.  The reference's printed value is that of some w in v [1 / (1 + delta),
    1 + delta], inside v [1 - delta, 1 + delta].

Rule: if a boundary lies in the closed interval v [1 - delta, 1 + delta] - which it does whenever the printed values of its two
ends differ - crosses is true.  Checked for boundaries k from 0 to 1.0001e6 (|e| <= (2^31 + 32768) / INT32_MAX ~= 1.000016 bounds
RMSE and MSD), values 0-4 ulps either side of each boundary and at the window's edges, lengths from 1 to 2^32 - 1.  And the
other way: the fallback stays rare (crosses false for >= 99 % of random values at n = 10^6)."""
from fractions import Fraction

import numpy as np
import pytest

from helpers import build_compare_round_driver, compare_round, exact_squares, exact_sum, reorder_bound

LENGTHS = [1, 2, 31, 8192, 524289, 10 ** 7, 2 ** 31, 2 ** 32 - 1]
MILLION = Fraction(10 ** 6)


def delta(n):
    """the reordering bound of the module docstring, exact"""
    return reorder_bound(n)


def boundary(k):
    return (Fraction(k) + Fraction(1, 2)) / MILLION


def printed(x):
    """'%f' of an exact non-negative rational: round half to even at six decimals (what glibc does on an exact binary value)"""
    q = x * MILLION
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return "%d.%06d" % divmod(f, 10 ** 6)


def boundary_inside(lo, hi):
    """some (k + 1/2) 1e-6 in [lo, hi]?"""
    k = (hi * MILLION - Fraction(1, 2)).__floor__()
    return k >= 0 and boundary(k) >= lo


def ulp_steps(v, steps):
    out = []
    for s in steps:
        w = v
        for _ in range(abs(s)):
            w = np.nextafter(w, np.inf if s > 0 else -np.inf)
        out.append(float(w))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_compare_round_driver(tmp_path_factory.mktemp("compare_round"))


def test_printed_matches_percent_f():
    """printed() is the '%f' of a double, on both sides of and on boundaries"""
    rng = np.random.default_rng(5)
    for k in [0, 1, 2, 499999, 999999, 1000000, 1000016] + [int(x) for x in rng.integers(0, 1000100, 200)]:
        b = float(boundary(k))
        for v in ulp_steps(b, range(-3, 4)) + [float(x) for x in rng.uniform(0, 1.0001, 20)]:
            assert printed(Fraction(v)) == "%f" % v, v


def test_bound_covers_the_reordering(driver):
    """compare_reorder_bound(n) >= delta(n) at every length, and not far above it (a wider window re-sums more streams)"""
    for (rel, _), n in zip(compare_round(driver, [(n, 0.0) for n in LENGTHS]), LENGTHS):
        d = delta(n)
        assert Fraction(rel) >= d, (n, rel, float(d))
        assert Fraction(rel) <= 2 * d + Fraction(1, 10 ** 14), (n, rel, float(d))


def test_crosses_whenever_the_order_could_show(driver):
    rng = np.random.default_rng(20261015)
    ks = sorted({0, 1, 2, 3, 9, 10, 99, 100, 210384, 499999, 500000, 999998, 999999, 1000000, 1000015, 1000016, 1000099, 1000100}
                | {int(x) for x in rng.integers(0, 1000101, 40)} | {int(x) for x in np.unique(np.geomspace(1, 1000100, 40).astype(int))})
    low = [0.0, 5e-324, 2.2250738585072014e-308, 1e-300, 1e-12, 1e-7, 4e-7, 4.99999e-7]
    rows, meta = [], []
    for n in LENGTHS:
        d = delta(n)
        for k in ks:
            b = boundary(k)
            near = float(b)
            vs = ulp_steps(near, range(-4, 5))
            for dd in (d, d * (1 - Fraction(1, 2 ** 20)), d * (1 + Fraction(1, 2 ** 20))):
                # v with v (1 - dd) == b or v (1 + dd) == b: the window's edges, and just inside / outside them
                for edge in (b / (1 - dd), b / (1 + dd)):
                    vs += ulp_steps(float(edge), range(-1, 2))
            for v in vs:
                rows.append((n, v))
                meta.append((n, d, k))
        for v in low:
            rows.append((n, v))
            meta.append((n, d, None))
    answers = compare_round(driver, rows)
    fired = ties = 0
    for (n, v), (_, d, k), (rel, crosses) in zip(rows, meta, answers):
        lo, hi = Fraction(v) * (1 - d), Fraction(v) * (1 + d)
        must = boundary_inside(lo, hi)
        assert must or printed(lo) == printed(hi)  # the closed-interval rule covers every change of the printed value
        if must:
            ties += 1
            assert crosses, (n, v.hex(), k, float(d), rel)
        fired += crosses
        if v < 4.5e-7:
            assert not crosses, (n, v)  # an error-free stream (or nearly) is never re-summed
    assert ties > len(rows) // 4 and fired < len(rows)  # both sides of the rule are exercised


def test_fallback_stays_rare(driver):
    rng = np.random.default_rng(77)
    vs = rng.uniform(1e-4, 1.0, 100000)
    answers = compare_round(driver, [(10 ** 6, v) for v in vs])
    assert sum(c for _, c in answers) <= 1000


def test_exact_sum_helpers():
    """the exact references of the GPU tests (helpers.exact_sum / exact_squares) against Fraction arithmetic"""
    rng = np.random.default_rng(3)
    e = np.concatenate([rng.uniform(-1.0001, 1.0001, 2000), rng.normal(0, 1e-6, 500), [0.0, 1 / 2147483647.0, -1.0, 2.0 ** -30]])
    want_sq = sum(Fraction(float(x)) ** 2 for x in e)
    assert sum(exact_sum(part) for part in exact_squares(e)) == want_sq
    assert exact_sum(np.abs(e)) == sum(abs(Fraction(float(x))) for x in e)
