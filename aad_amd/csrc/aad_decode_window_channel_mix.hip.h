/*
 * aad_decode_window_channel_mix.hip.h - window decode over a corpus of mono and stereo streams into rows of ONE channel count
 * (AADHip_ChannelMixWindowDecodePlanCreate -> AADHip_WindowDecodePlanRun).
 *
 * The mixed-format run (aad_decode_window_mixed.hip.h) with the source channel count as one more part of the kernel variant: one
 * launch per (source channels, bits, mid/side) present in the plan - the six stereo variants, then mono 4-, 3- and 2-bit, at most
 * nine (aad_launch_policy.h channel_mix_variants, plan_channel_mix_window_decode).  A launch's lanes are (window, block-in-window,
 * SOURCE channel); a lane reads its window, then its stream's 8-byte ChannelStreamFormat record and leaves when the stream
 * belongs to another variant - per window, so a stereo pair leaves together.  Where the source's channel count is not the
 * output's, window_lane's OUTC mode takes the mix in `finish`, in front of every store (header samples, wide chunks, the byte-load
 * tail; zeros go the same way):
 *   mono -> 2 rows: the lane stores every sample into both rows;
 *   stereo -> 1 row: the pair exchanges the finished L / R sample through pair_swap - the neighbouring lane, of the same window
 *     and block, with the same trip counts, as for the inverse mid/side - and lane c == 0 alone stores (L + R) >> 1 as int16 or
 *     (float)(L + R) * 2^-16 as float32.
 *
 * Every element of the output is written exactly once per run: a window by the launch of its stream's variant, a window whose
 * stream index is out of range (zeros in all the output's rows) by the run's first launch, whatever its source channel count.
 */
#ifndef AAD_DECODE_WINDOW_CHANNEL_MIX_HIP_H
#define AAD_DECODE_WINDOW_CHANNEL_MIX_HIP_H

#include "aad_decode_window.hip.h"

namespace aad {

struct ChannelMixWindowArgs {
  WindowArgs w;                       /* channels: the variant's SOURCE count; samples_per_block: its smallest; block_size unused */
  const ChannelStreamFormat *formats; /* [w.num_streams] */
  uint32_t owns_strays;               /* this launch writes the windows whose stream is out of range */
  uint32_t out_channels;              /* 1 or 2: the rows of a window */
};

template <int BITS, int CHF, bool MS, int ST, int OUTC>
__global__ void __launch_bounds__(256) decode_window_channel_mix_kernel(ChannelMixWindowArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x; /* a multiple of 64: the lanes of a channel pair stay neighbours */
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true, OUTC>(a.w, lds, lane, a.formats, a.owns_strays);
}

} /* namespace aad */

#endif /* AAD_DECODE_WINDOW_CHANNEL_MIX_HIP_H */
