/* aad_decode_window_channel_mix_placed.hip - translation unit of the channel-mix window decoder with a span per window
 * (aad_decode_window_placed.hip.h).  AAD_WINDOW_HALF=0: float32 rows alone. */
#include "aad_decode_window_placed.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS, int ST, int OUTC>
static void launch_bits(const ChannelMixWindowPlacedArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.g.m.w.channels == 1)
    AAD_LAUNCH((decode_window_channel_mix_placed_kernel<BITS, 1, false, ST, OUTC>), grid, block, lds, stream, a);
  else if (a.g.m.w.mid_side)
    AAD_LAUNCH((decode_window_channel_mix_placed_kernel<BITS, 2, true, ST, OUTC>), grid, block, lds, stream, a);
  else
    AAD_LAUNCH((decode_window_channel_mix_placed_kernel<BITS, 2, false, ST, OUTC>), grid, block, lds, stream, a);
}

template <int ST, int OUTC>
static void launch_type(const ChannelMixWindowPlacedArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.g.m.w.bits == 4) launch_bits<4, ST, OUTC>(a, grid, block, lds, stream);
  else if (a.g.m.w.bits == 3) launch_bits<3, ST, OUTC>(a, grid, block, lds, stream);
  else launch_bits<2, ST, OUTC>(a, grid, block, lds, stream);
}

template <int ST>
static void launch_rows(const ChannelMixWindowPlacedArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.g.m.out_channels == 1) launch_type<ST, 1>(a, grid, block, lds, stream);
  else launch_type<ST, 2>(a, grid, block, lds, stream);
}

/* one launch of a run: args.w.channels / args.w.bits / args.w.mid_side name the variant, args.out_channels (1 or 2) the output */
template <>
void launch_decode_window_channel_mix_placed_unit<AAD_WINDOW_HALF != 0>(
    const ChannelMixWindowArgs &args, const struct AADHipWindowSpan *spans, const float *gain, uint32_t add, const WindowLaunch &p,
    int32_t sample_type, hipStream_t stream)
{
  const ChannelMixWindowPlacedArgs a = {{args, gain, add, 0}, reinterpret_cast<const uint64_t *>(spans)};
  const dim3 grid(p.grid), block(p.workgroup);
#if AAD_WINDOW_HALF
  if (sample_type == AAD_HIP_SAMPLE_BFLOAT16) launch_rows<AAD_HIP_SAMPLE_BFLOAT16>(a, grid, block, p.lds, stream);
  else launch_rows<AAD_HIP_SAMPLE_FLOAT16>(a, grid, block, p.lds, stream);
#else
  (void)sample_type;
  launch_rows<AAD_HIP_SAMPLE_FLOAT32>(a, grid, block, p.lds, stream);
#endif
}

} /* namespace aad */
