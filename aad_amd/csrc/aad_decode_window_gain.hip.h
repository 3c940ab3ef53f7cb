/*
 * aad_decode_window_gain.hip.h - window decode with a per-window gain, written or added into float rows
 * (AADHip_WindowDecodePlanRunGain).
 *
 * The three window decode kernels (aad_decode_window.hip.h, aad_decode_window_mixed.hip.h, aad_decode_window_channel_mix.hip.h)
 * with window_lane's GAIN mode: same lanes, same K, same variants, same reads of the corpus.  A lane reads its window's gain g once
 * (one float beside the two words of the window) and its row writer turns the float32 value f of a plain run into
 *   STORE: p = fl32(g * f)            ADD: fl32(old + p), old the element's content - float16 / bfloat16: widened, exact -
 * and then into the row's type by the one rounding of pack_half2.  The multiply and the add are two instructions (WindowRow::gained,
 * ::sum: contraction off, the product a register value of its own), never an fma and never a mixed-precision fma in front of the
 * float16 pack, so every element is torch's (out.float() + gain[:, None, None] * row_float32).to(dtype) bit for bit.  STORE / ADD
 * is a flag in the row, uniform over the run, as WindowLevels<true>::store: one set of kernels.
 *
 * A whole 16-sample chunk stays on the vector path: under ADD the old chunk is loaded as 16-byte vectors at the row's own (4- or
 * 2-byte) alignment - four for float32, two for the 16-bit types - in front of the chunk's decode (WindowRow::fetch: the loads are
 * in flight while the lane decodes), added in float32 and stored by the plain kernels' vector stores; the two rows of a mono
 * source in a two-channel output are loaded, added and stored each on its own.  The head and tail of a row
 * and the frames the stream does not produce go element by element, the latter as g * 0 (STORE: -0 under a negative gain) or
 * old + g * 0.  Every element is read at most once and written exactly once per run, by one lane.
 */
#ifndef AAD_DECODE_WINDOW_GAIN_HIP_H
#define AAD_DECODE_WINDOW_GAIN_HIP_H

#include "aad_decode_window_channel_mix.hip.h"
#include "aad_decode_window_mixed.hip.h"

namespace aad {

/* gain: [num_windows] float, or null (every gain is 1); add: AAD_HIP_WINDOW_GAIN_ADD */
struct WindowGainArgs {
  WindowArgs w;
  const float *gain;
  uint32_t add;
  uint32_t reserved;
};
struct MixedWindowGainArgs {
  MixedWindowArgs m;
  const float *gain;
  uint32_t add;
  uint32_t reserved;
};
struct ChannelMixWindowGainArgs {
  ChannelMixWindowArgs m;
  const float *gain;
  uint32_t add;
  uint32_t reserved;
};

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_gain_kernel(WindowGainArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x; /* a multiple of 64: the lanes of a channel pair stay neighbours */
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, false, 0, StreamFormat, false, true>(a.w, lds, lane, nullptr, 0, nullptr, a.gain, a.add);
}

template <int BITS, int CHF, bool MS, int ST>
__global__ void __launch_bounds__(256) decode_window_mixed_gain_kernel(MixedWindowGainArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true, 0, StreamFormat, false, true>(a.m.w, lds, lane, a.m.formats, a.m.owns_strays, nullptr,
                                                                      a.gain, a.add);
}

template <int BITS, int CHF, bool MS, int ST, int OUTC>
__global__ void __launch_bounds__(256) decode_window_channel_mix_gain_kernel(ChannelMixWindowGainArgs a)
{
  __shared__ __attribute__((aligned(16))) char lds[kLdsBytesDenseDec];
  stage_tables<BITS, false>(lds);
  stage_dense_decode_tables<BITS>(lds);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; lane < a.m.w.lanes; lane += stride)
    window_lane<BITS, CHF, MS, ST, true, OUTC, ChannelStreamFormat, false, true>(a.m.w, lds, lane, a.m.formats, a.m.owns_strays,
                                                                                nullptr, a.gain, a.add);
}

} /* namespace aad */

#endif /* AAD_DECODE_WINDOW_GAIN_HIP_H */
