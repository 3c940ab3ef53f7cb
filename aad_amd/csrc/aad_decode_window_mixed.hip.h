/*
 * aad_decode_window_mixed.hip.h - window decode over a corpus whose streams do not share a format
 * (AADHip_MixedWindowDecodePlanCreate -> AADHip_WindowDecodePlanRun).
 *
 * The step tables in LDS and the chunk bodies are per BITS and mid/side is a template parameter, so a run is one launch per kernel
 * VARIANT (bits, mid/side) present in the plan - at most six for stereo, three otherwise (aad_launch_policy.h window_variants,
 * plan_mixed_window_decode).  Every launch walks all the windows with window_lane's lanes (aad_decode_window.hip.h): a lane reads
 * its window, then its stream's 8-byte StreamFormat record, takes samples_per_block and block_size from the record and leaves at
 * once when the stream belongs to another variant.  The stream is a property of the window, so a window's lanes leave together
 * and a mid/side pair stays on neighbouring lanes.  A launch's K comes from the smallest block among its variant's streams; the
 * lanes past a longer-blocked stream's own last covering block leave as the lanes past a window's last block always did.
 *
 * Every element of the output is written exactly once per run: a window by the launch of its stream's variant, a window whose
 * stream index is out of range (all zeros) by the run's first launch (owns_strays).
 */
#ifndef AAD_DECODE_WINDOW_MIXED_HIP_H
#define AAD_DECODE_WINDOW_MIXED_HIP_H

#include "aad_decode_window.hip.h"

namespace aad {

struct MixedWindowArgs {
  WindowArgs w;                /* samples_per_block: the variant's smallest (blocks_per_window follows from it); block_size unused */
  const StreamFormat *formats; /* [w.num_streams] */
  uint32_t owns_strays;        /* this launch writes the windows whose stream is out of range */
  uint32_t reserved;
};

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_mixed_kernel(MixedWindowArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x; /* a multiple of 64: the lanes of a channel pair stay neighbours */
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true>(a.w, lds, lane, a.formats, a.owns_strays);
}

} /* namespace aad */

#endif /* AAD_DECODE_WINDOW_MIXED_HIP_H */
