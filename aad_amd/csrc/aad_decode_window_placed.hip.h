/*
 * aad_decode_window_placed.hip.h - window decode with a span per window: a crop of L frames placed at element o of its row
 * (AADHip_WindowDecodePlanRunPlaced: float rows with a gain, stored or added; AADHip_WindowDecodePlanRunPlacedStats: the level
 * statistics of the crop alone, no rows).
 *
 * The gain and the statistics kernels (aad_decode_window_gain.hip.h, aad_decode_window_stats.hip.h) with window_lane's PLACED
 * mode: same lanes, same K, same variants as the run without spans for the same T.  A lane reads its window's span (two words
 * beside the two of the window; a null table: (T, 0)), clips it to Le = 0 for o >= T, else min(L, T - o) (aad_window_span.h), and
 * runs its crop arithmetic over Le instead of T - the early leave, hi, n, count - with its row writer at the row's element o; the
 * row pitch stays T.  Lane k decodes block first_frame / spb + k as ever, so a short span leaves most of a window's K lanes
 * without a block.
 *
 * The fill.  Under STORE the elements of [0, T) outside the span become +0 (not g * 0).  They are written by all K lanes of the
 * window: each takes the tile it owns in a run without spans, [k * spb - phase, (k + 1) * spb - phase) cut to [0, T), minus the
 * span - at most two pieces and at most spb elements (window_fill_tile) - in front of its early leave, 16 elements at a time by
 * the chunk path's 16-byte stores at the row's own alignment where that many remain (WindowRow::fill).  The tiles cover [0, T)
 * because K is planned from the variant's smallest spb.  The R lane of a down-mixed pair fills nothing, a twin fills both rows,
 * and in a mixed or channel-mix run the launch that owns the window - for a stray window the one that owns_strays - fills it.
 * Under ADD nothing outside the span is read or written.  Every element is written at most once per run, by one lane, under
 * STORE exactly once.
 *
 * The statistics kernels write no rows (out is null), so one sample type serves: they are instantiated for int16 alone, whose
 * down-mix statistic is the floor mix's as for every type.
 */
#ifndef AAD_DECODE_WINDOW_PLACED_HIP_H
#define AAD_DECODE_WINDOW_PLACED_HIP_H

#include "aad_decode_window_gain.hip.h"
#include "aad_decode_window_stats.hip.h"

namespace aad {

/* spans: [num_windows][2] uint64 (struct AADHipWindowSpan: num_frames, out_frame), or null - every span is (T, 0) */
struct WindowPlacedArgs {
  WindowGainArgs g;
  const uint64_t *spans;
};
struct MixedWindowPlacedArgs {
  MixedWindowGainArgs g;
  const uint64_t *spans;
};
struct ChannelMixWindowPlacedArgs {
  ChannelMixWindowGainArgs g;
  const uint64_t *spans;
};
struct WindowPlacedStatsArgs {
  WindowStatsArgs s; /* s.w.out is null */
  const uint64_t *spans;
};
struct MixedWindowPlacedStatsArgs {
  MixedWindowStatsArgs s;
  const uint64_t *spans;
};
struct ChannelMixWindowPlacedStatsArgs {
  ChannelMixWindowStatsArgs s;
  const uint64_t *spans;
};

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_placed_kernel(WindowPlacedArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x; /* a multiple of 64: the lanes of a channel pair stay neighbours */
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.g.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, false, 0, StreamFormat, false, true, true>(a.g.w, lds, lane, nullptr, 0, nullptr, a.g.gain,
                                                                            a.g.add, a.spans);
}

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_mixed_placed_kernel(MixedWindowPlacedArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.g.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true, 0, StreamFormat, false, true, true>(a.g.m.w, lds, lane, a.g.m.formats, a.g.m.owns_strays,
                                                                           nullptr, a.g.gain, a.g.add, a.spans);
}

template <int BITS, int CHF, bool MS, int ST, int OUTC>
__global__ void __launch_bounds__(256) decode_window_channel_mix_placed_kernel(ChannelMixWindowPlacedArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.g.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true, OUTC, ChannelStreamFormat, false, true, true>(
        a.g.m.w, lds, lane, a.g.m.formats, a.g.m.owns_strays, nullptr, a.g.gain, a.g.add, a.spans);
}

template <int BITS, int CHF, bool MS>
__global__ void __launch_bounds__(256) decode_window_placed_stats_kernel(WindowPlacedStatsArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.s.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, kRowI16, false, 0, StreamFormat, true, false, true>(a.s.w, lds, lane, nullptr, 0, a.s.stats, nullptr, 0,
                                                                                 a.spans);
}

template <int BITS, int CHF, bool MS>
__global__ void __launch_bounds__(256) decode_window_mixed_placed_stats_kernel(MixedWindowPlacedStatsArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.s.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, kRowI16, true, 0, StreamFormat, true, false, true>(a.s.m.w, lds, lane, a.s.m.formats,
                                                                                a.s.m.owns_strays, a.s.stats, nullptr, 0, a.spans);
}

template <int BITS, int CHF, bool MS, int OUTC>
__global__ void __launch_bounds__(256) decode_window_channel_mix_placed_stats_kernel(ChannelMixWindowPlacedStatsArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.s.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, kRowI16, true, OUTC, ChannelStreamFormat, true, false, true>(
        a.s.m.w, lds, lane, a.s.m.formats, a.s.m.owns_strays, a.s.stats, nullptr, 0, a.spans);
}

} /* namespace aad */

#endif /* AAD_DECODE_WINDOW_PLACED_HIP_H */
