/* aad_resample.h - the arithmetic of the resample stage behind a window decode (AADHip_Resampler*, include/aad_hip.h "resample"),
 * compiled for the host and for the device: the reduction of a ratio and what a resampler refuses, the integer polyphase bank
 * (built on the host in double precision), the source batch's row length and the per-window resolve, which the resolve kernel
 * (aad_resample.hip) runs once per window, and a row's span and `count` for the runs with spans and statistics.  A CPU test runs
 * the same functions against a numpy restatement of the definition (tests/resample_policy_driver.cpp, tests/resample_oracle.py;
 * tests/resample_mix_driver.cpp against a brute force; tests/resample_wide_driver.cpp for the limits of a wide resampler and the
 * gather plan of its kernels, at the end of this file).  Plain C++ with no container, as aad_windows.h. */
#ifndef AAD_RESAMPLE_H
#define AAD_RESAMPLE_H

#include <math.h>
#include <stdint.h>

#include "aad_window_span.h"

#if defined(__HIPCC__)
#define AAD_RESAMPLE_FN __host__ __device__ inline
#else
#define AAD_RESAMPLE_FN inline
#endif

namespace aad {

constexpr uint32_t kResampleUnity = 16384;        /* Q14: every phase sums to it */
constexpr uint32_t kResampleMaxPhases = 1024;     /* L */
constexpr uint32_t kResampleMaxTaps = 256;        /* K */
constexpr uint32_t kResampleMaxBankBytes = 65536; /* 2 L K */
constexpr uint32_t kResampleMaxAbsSum = 65535;    /* sum |h| of a phase: 32768 * 65535 < 2^31, int32 accumulators are exact */
constexpr uint32_t kResampleNoBank = 0xFFFF;      /* a select entry, a lane's bank: the row is zeros */
/* AADHip_ResamplerCreateWide: K, sum |h| and the definitions as above; L and the bank are bounded by the 32-bit indices alone */
constexpr uint32_t kResampleWideMaxPhases = 32768;       /* L */
constexpr uint32_t kResampleWideMaxBankBytes = 2u << 20; /* 2 L K */
constexpr uint64_t kResampleMaxCoefficients = 1ull << 31; /* all banks of a resampler: ResampleBankDesc::offset is 32-bit */

/* ---- ratio -------------------------------------------------------------------------------------------------------------------- */

struct ResampleRatio {
  uint32_t L, M; /* output rate / source rate = L / M, reduced */
};

/* false for up == 0 or down == 0 */
inline bool resample_reduce(uint32_t up, uint32_t down, ResampleRatio *r)
{
  if (up == 0 || down == 0) return false;
  uint32_t a = up, b = down;
  while (b != 0) {
    const uint32_t t = a % b;
    a = b;
    b = t;
  }
  r->L = up / a;
  r->M = down / a;
  return true;
}

/* K: 2 for the identity, else 2 * ceil(12 / s) with s = min(1, L / M) - twelve zero crossings of the low-pass on either side */
inline uint64_t resample_taps(uint32_t L, uint32_t M)
{
  if (L == 1 && M == 1) return 2;
  if (L >= M) return 24;
  return 2 * ((12ull * M + L - 1) / L);
}

/* what creation refuses before it builds the bank: L, K and the bank's bytes */
inline bool resample_shape_ok(uint32_t L, uint32_t M)
{
  if (L > kResampleMaxPhases) return false;
  const uint64_t K = resample_taps(L, M);
  return K <= kResampleMaxTaps && 2ull * L * K <= kResampleMaxBankBytes;
}

/* what AADHip_ResamplerCreateWide refuses before it builds the bank; everything resample_shape_ok accepts passes */
inline bool resample_wide_shape_ok(uint32_t L, uint32_t M)
{
  if (L > kResampleWideMaxPhases) return false;
  const uint64_t K = resample_taps(L, M);
  return K <= kResampleMaxTaps && 2ull * L * K <= kResampleWideMaxBankBytes;
}

/* resample_shape_ok from a bank's own (L, K): the FIR kernels of a wide resampler keep such a bank whole in LDS ("resident") and
 * gather the rows of any other per round of outputs */
AAD_RESAMPLE_FN bool resample_bank_resident(uint32_t L, uint32_t K)
{
  return L <= kResampleMaxPhases && K <= kResampleMaxTaps && 2ull * L * K <= kResampleMaxBankBytes;
}

/* ---- bank --------------------------------------------------------------------------------------------------------------------- */

inline double resample_bessel_i0(double x)
{
  const double q = x * x / 4;
  double term = 1, sum = 1;
  for (int k = 1; k < 200 && term > 1e-18 * sum; k++) {
    term *= q / ((double)k * k);
    sum += term;
  }
  return sum;
}

/* g(t), t = num / L: 0.94 s sinc(0.94 s t) I0(9 sqrt(1 - (t / (K/2))^2)) / I0(9), 0 where |t| > K/2.  Even in t by construction. */
inline double resample_prototype(int64_t num, uint32_t L, uint32_t M, uint32_t K)
{
  const double pi = 3.14159265358979323846;
  const double t = fabs((double)num / (double)L), half = K / 2;
  if (t > half) return 0;
  const double s = L >= M ? 1.0 : (double)L / (double)M, c = 0.94 * s, x = pi * c * t;
  const double sinc = x == 0 ? 1.0 : sin(x) / x;
  const double u = 1 - (t / half) * (t / half);
  return c * sinc * resample_bessel_i0(9 * sqrt(u > 0 ? u : 0)) / resample_bessel_i0(9);
}

/* Phase p of the bank into h[K].  Tap k sits at t = k - (K/2 - 1) - p / L, kept as the exact numerator (k - (K/2 - 1)) L - p so
 * that phases p and L - p are mirror images to the last bit: the sum that scales the phase to 16384 runs from the middle outwards,
 * by |t|, the same order in both.  Then floors, and 1 more to the 16384 - sum(floors) taps with the largest fractional parts, ties
 * to the lower k.  Returns sum |h|. */
inline uint32_t resample_build_phase(uint32_t L, uint32_t M, uint32_t K, uint32_t p, int16_t *h)
{
  double g[kResampleMaxTaps], frac[kResampleMaxTaps];
  int32_t fl[kResampleMaxTaps];
  const int64_t lead = (int64_t)K / 2 - 1;
  if (L == 1 && M == 1) {
    h[0] = (int16_t)kResampleUnity;
    h[1] = 0;
    return kResampleUnity;
  }
  for (uint32_t k = 0; k < K; k++) g[k] = resample_prototype(((int64_t)k - lead) * L - p, L, M, K);
  /* num < 0 for k <= lead when p > 0, for k < lead when p == 0 */
  int64_t right = p == 0 ? lead : lead + 1, left = right - 1;
  double sum = 0;
  while (left >= 0 || right < (int64_t)K) {
    const int64_t nl = left >= 0 ? -((left - lead) * (int64_t)L - p) : INT64_MAX;
    const int64_t nr = right < (int64_t)K ? (right - lead) * (int64_t)L - p : INT64_MAX;
    if (nr <= nl) sum += g[right++];
    else sum += g[left--];
  }
  int64_t total = 0;
  for (uint32_t k = 0; k < K; k++) {
    const double v = g[k] * (double)kResampleUnity / sum, f = floor(v);
    fl[k] = (int32_t)f;
    frac[k] = v - f;
    total += fl[k];
  }
  int64_t rest = (int64_t)kResampleUnity - total;
  if (rest < 0) rest = 0;
  if (rest > (int64_t)K) rest = K;
  for (; rest > 0; rest--) {
    uint32_t best = 0;
    for (uint32_t k = 1; k < K; k++)
      if (frac[k] > frac[best]) best = k;
    fl[best] += 1;
    frac[best] = -1;
  }
  uint32_t abs_sum = 0;
  for (uint32_t k = 0; k < K; k++) {
    h[k] = (int16_t)fl[k];
    abs_sum += (uint32_t)(fl[k] < 0 ? -fl[k] : fl[k]);
  }
  return abs_sum;
}

/* the bank of (L, M), L phases of K = resample_taps(L, M) taps into h[L * K] (resample_shape_ok held); false when a phase has
 * sum |h| > 65535 */
inline bool resample_build_bank(uint32_t L, uint32_t M, int16_t *h)
{
  const uint32_t K = (uint32_t)resample_taps(L, M);
  for (uint32_t p = 0; p < L; p++)
    if (resample_build_phase(L, M, K, p, h + (uint64_t)p * K) > kResampleMaxAbsSum) return false;
  return true;
}

/* ---- rows --------------------------------------------------------------------------------------------------------------------- */

/* frames of the source row that T output frames of bank (L, M, K) read: ((T - 1) M) div L + K; false for T == 0 and for
 * (T - 1) M >= 2^31 (the kernels index with 32 bits) */
inline bool resample_source_frames(uint32_t frames, uint32_t L, uint32_t M, uint32_t K, uint64_t *source_frames)
{
  if (frames == 0 || (uint64_t)(frames - 1) * M >= (1ull << 31)) return false;
  *source_frames = (uint64_t)(frames - 1) * M / L + K;
  return true;
}

/* one window's lane record: a contiguous torch int32 [N, 2] tensor on the device is the table */
struct ResampleLane {
  uint32_t bank;  /* index of the window's bank, kResampleNoBank: the row is zeros */
  uint32_t shift; /* first_frame - src_first: the source row's element that is the window's first frame */
};

struct ResampleResolved {
  uint64_t stream, src_first; /* the source window */
  ResampleLane lane;
};

/* Window {stream, first_frame} of variant `variant` (the int64 of the table read as uint64, so that a negative one is past V):
 * bank = select[stream][variant], none for a stream index >= num_streams, a variant >= variants and the entry kResampleNoBank.
 * The source window starts lead[bank] = K/2 - 1 frames early, or at frame 0 when the window starts inside that lead, and `shift`
 * says by how much.  A window without a bank keeps its own start: its source row is decoded and never read. */
AAD_RESAMPLE_FN ResampleResolved resample_resolve(uint64_t stream, uint64_t first_frame, uint64_t variant, uint64_t num_streams,
                                                  uint32_t variants, const uint16_t *select, const uint16_t *lead)
{
  ResampleResolved r;
  r.stream = stream;
  r.src_first = first_frame;
  r.lane.bank = kResampleNoBank;
  r.lane.shift = 0;
  if (stream >= num_streams || variant >= variants) return r;
  const uint32_t bank = select[stream * variants + variant];
  if (bank == kResampleNoBank) return r;
  const uint64_t before = first_frame < lead[bank] ? first_frame : lead[bank];
  r.src_first = first_frame - before;
  r.lane.bank = bank;
  r.lane.shift = (uint32_t)before;
  return r;
}

/* ---- rows with spans and statistics (AADHip_ResamplerRunGain, AADHip_ResamplerRunStats) ---------------------------------------- */

/* Le: the OUTPUT frames of span (L_span, o) that a row of T elements takes - the rule of window decode with spans, not a second one */
AAD_RESAMPLE_FN uint64_t resample_span_frames(uint64_t num_frames, uint64_t out_frame, uint32_t frames)
{
  return window_span_frames(num_frames, out_frame, frames);
}

/* `count` of a resampled row: the number of n < Le whose centre source frame, element shift + (n M) div L of the source row, the
 * stream had - c_src being the source row's own count (AADHip_WindowDecodePlanRunStats over the source windows), never more than
 * the row's length.  shift + (n M) div L < c  <=>  n M < (c - shift) L  <=>  n < ceil((c - shift) L / M); c < 2^32 and L <= 32768
 * (a wide resampler's largest), so the product is below 2^47 and 64 bits hold it with M added. */
AAD_RESAMPLE_FN uint64_t resample_output_count(uint64_t c_src, uint32_t source_frames, uint32_t shift, uint32_t L, uint32_t M,
                                               uint64_t Le)
{
  const uint64_t c = c_src < source_frames ? c_src : source_frames;
  if (c <= shift) return 0;
  const uint64_t n = ((c - shift) * L + M - 1) / M;
  return n < Le ? n : Le;
}

/* ---- LDS of the FIR kernels (aad_resample_tile.hip.h, aad_resample_wide.hip) ---------------------------------------------------- */

constexpr uint32_t kResampleThreads = 256;
constexpr uint32_t kResamplePerThread = 4;
constexpr uint32_t kResampleTile = kResampleThreads * kResamplePerThread; /* outputs of one workgroup's tile */

/* int16 elements between two phases of a bank in LDS: adjacent outputs read different phases, each its K taps as K/2 words in
 * step, so the phases' rows start an odd number of words apart - p -> p * stride / 2 mod 32 then maps 32 phases onto 32 banks */
AAD_RESAMPLE_FN uint32_t resample_lds_stride(uint32_t K) { return (K / 2) % 2 == 0 ? K + 2 : K; }
/* int16 elements of a tile's span of the source row: the frames from the first output's first tap to the last output's last,
 * one in front for the 4-byte alignment of the row's loads, and the word a thread at an odd element reads past its last tap */
inline uint64_t resample_span_elements(uint32_t L, uint32_t M, uint32_t K)
{
  return ((((uint64_t)(kResampleTile - 1) * M) / L + 1 + K + 1 + 2) + 1) / 2 * 2;
}
/* bytes of LDS of a workgroup whose bank is (L, M, K), the bank whole */
inline uint64_t resample_lds_bytes(uint32_t L, uint32_t M, uint32_t K)
{
  return 2 * ((uint64_t)L * resample_lds_stride(K) + resample_span_elements(L, M, K));
}

/* The gather path of a wide resampler's kernels.  A tile is walked in rounds of R consecutive outputs, and a round has in LDS one
 * bank row per output - resample_lds_stride(K) int16 - and the output's phase, a 32-bit word: 2 * stride + 4 bytes an output.  R is
 * the largest of 256, 128 and 64 whose rows and phases stay within kResampleGatherBytes: small enough that, with a span of a few
 * KB, three or four workgroups share a CU's 160 KB and run through each other's barriers; 64 always fits (K = 256: 64 * 520 bytes).
 * 256 is the tile's 256 threads with one output each; a smaller R leaves the other waves only the copy. */
constexpr uint32_t kResampleGatherBytes = 40960;
constexpr uint32_t kResampleMaxRound = kResampleThreads;
inline uint32_t resample_gather_round(uint32_t K)
{
  uint32_t R = kResampleMaxRound;
  while (R > 64 && (uint64_t)R * (2 * resample_lds_stride(K) + 4) > kResampleGatherBytes) R /= 2;
  return R;
}
/* int16 elements between two rows of a gathered bank in DEVICE memory: rows on 16-byte boundaries, so that the copy reads them
 * with 16-byte loads - a quarter of the load instructions, which are what the copy costs.  The bank on the host, which
 * AADHip_ResamplerBank returns, and a resident bank on the device keep their rows K apart. */
AAD_RESAMPLE_FN uint32_t resample_gather_pitch(uint32_t K) { return (K + 7u) & ~7u; }
/* Output u of a tile - thread tid's j-th output is u = tid + 256 j - belongs to round u / R of the tile and is row u mod R of it: R
 * is a power of two.  The kernel publishes the output's phase at index[row] and reads its taps from row `row` of the round. */
struct ResampleGatherSlot {
  uint32_t round, row;
};
AAD_RESAMPLE_FN ResampleGatherSlot resample_gather_slot(uint32_t u, uint32_t R)
{
  return ResampleGatherSlot{u >> __builtin_ctz(R), u & (R - 1)};
}
/* what a gathered bank (L, M, K) needs of LDS at round R: { rows, phase index, span } in bytes */
struct ResampleGatherLds {
  uint64_t rows, index, span;
};
inline ResampleGatherLds resample_gather_lds(uint32_t L, uint32_t M, uint32_t K, uint32_t R)
{
  return ResampleGatherLds{2ull * R * resample_lds_stride(K), 4ull * R, 2 * resample_span_elements(L, M, K)};
}

} /* namespace aad */

#endif /* AAD_RESAMPLE_H */
