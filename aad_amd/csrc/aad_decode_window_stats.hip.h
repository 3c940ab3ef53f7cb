/*
 * aad_decode_window_stats.hip.h - window decode with exact per-row level statistics (AADHip_WindowDecodePlanRunStats).
 *
 * The three window decode kernels (aad_decode_window.hip.h, aad_decode_window_mixed.hip.h, aad_decode_window_channel_mix.hip.h)
 * with window_lane's STATS mode: same lanes, same K, same variants, same reads and - when the run has rows - the same stores.  A
 * lane sums v * v and |v| and keeps the largest |v| over the samples it keeps, v being the int16 value of the row whatever the
 * sample type (a float down-mix row holds (L + R) * 2^-16 - float16 / bfloat16: rounded - its statistic is that of
 * (L + R) >> 1), in 64-bit accumulators:
 * a 16-sample chunk at full scale is 2^34 in sum_sq and a 2-bit block of 65535 bytes 2^33 in sum_abs.  A row's samples come from
 * up to K lanes that need not share a wave, a workgroup or - in a mixed plan - anything but the launch: the run clears the table
 * on the stream and every lane that kept a non-zero sample ends with two 64-bit atomic adds and one atomic max into its row's
 * AADHipRowStats (vector-memory atomics without return; about K per row beside ~spb decoded samples per lane).  `count` comes
 * from the stream table alone and is added by the lane of the window's first block, which always exists.  Stray windows, rows of
 * silence and the windows past a stream's end keep the zeros of the clear.
 *
 * out == null: a statistics-only run.  The test is uniform over the run; the range logic is the row-writing run's.
 */
#ifndef AAD_DECODE_WINDOW_STATS_HIP_H
#define AAD_DECODE_WINDOW_STATS_HIP_H

#include "aad_decode_window_channel_mix.hip.h"
#include "aad_decode_window_mixed.hip.h"

namespace aad {

static_assert(sizeof(AADHipRowStats) == 4 * sizeof(unsigned long long), "statistics record layout");

/* stats: [num_windows][rows of a window] AADHipRowStats, cleared in front of the run's first launch */
struct WindowStatsArgs {
  WindowArgs w; /* w.out may be null */
  unsigned long long *stats;
};
struct MixedWindowStatsArgs {
  MixedWindowArgs m;
  unsigned long long *stats;
};
struct ChannelMixWindowStatsArgs {
  ChannelMixWindowArgs m;
  unsigned long long *stats;
};

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_stats_kernel(WindowStatsArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x; /* a multiple of 64: the lanes of a channel pair stay neighbours */
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, false, 0, StreamFormat, true>(a.w, lds, lane, nullptr, 0, a.stats);
}

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_mixed_stats_kernel(MixedWindowStatsArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true, 0, StreamFormat, true>(a.m.w, lds, lane, a.m.formats, a.m.owns_strays, a.stats);
}

template <int BITS, int CHF, bool MS, int ST, int OUTC>
__global__ void __launch_bounds__(256) decode_window_channel_mix_stats_kernel(ChannelMixWindowStatsArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true, OUTC, ChannelStreamFormat, true>(a.m.w, lds, lane, a.m.formats, a.m.owns_strays, a.stats);
}

} /* namespace aad */

#endif /* AAD_DECODE_WINDOW_STATS_HIP_H */
