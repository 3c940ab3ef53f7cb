/* aad_compare_round.h - when may the order of the reconstruction statistics' fp64 sums show in the line `aad -c` prints?
 * compare_finish_kernel (aad_compare.hip.h) asks this of its tree-order RMSE and MSD, and re-sums a stream in the reference's
 * order when the answer is yes.  Device and host share this header so that a CPU test proves the rule with exact arithmetic
 * (tests/test_compare_round.py, through tests/compare_round_driver.cpp).
 *
 * Sums of n non-negative terms agree with their exact value to gamma_{n-1} = (n-1) u / (1 - (n-1) u) relative in any order
 * (u = 2^-53); two orders, the correctly rounded division by n and, for the RMSE, the square root widen that to delta(n)
 * ~= 2 n u (the test derives delta exactly).  compare_reorder_bound(n) >= delta(n) for every n a stream can have, and
 * compare_crosses_boundary(v, rel) is true whenever a rounding boundary (k + 1/2) 1e-6 of the six printed decimals lies in
 * v (1 +- rel).  Contraction is off: the same products and sums, rounded the same way, on the device and the host. */
#ifndef AAD_COMPARE_ROUND_H
#define AAD_COMPARE_ROUND_H

#include <math.h>

#if defined(__HIPCC__)
#define AAD_COMPARE_ROUND_FN __host__ __device__ inline
#else
#define AAD_COMPARE_ROUND_FN inline
#endif

namespace aad {

/* relative distance the reference's order may put between its RMSE / MSD and the tree's, for n values (the CLI's uint32 count) */
AAD_COMPARE_ROUND_FN double compare_reorder_bound(double n)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return 2.5 * n * 1.1102230246251565e-16 + 1e-15;
}

/* a %f rounding boundary inside v (1 +- rel)? */
AAD_COMPARE_ROUND_FN bool compare_crosses_boundary(double v, double rel)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double lo = v * (1.0 - rel) * 1e6, hi = v * (1.0 + rel) * 1e6;
  return floor(lo + 0.5 - 1e-9) != floor(hi + 0.5 + 1e-9); /* the 1e-9: the products above are rounded themselves */
}

} /* namespace aad */

#undef AAD_COMPARE_ROUND_FN

#endif /* AAD_COMPARE_ROUND_H */
