/* aad_decode_window_channel_mix.hip - translation unit of the channel-mix window decoder (aad_decode_window_channel_mix.hip.h). */
#include "aad_decode_window_channel_mix.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS, int ST, int OUTC>
static void launch_bits(const ChannelMixWindowArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.w.channels == 1)
    AAD_LAUNCH((decode_window_channel_mix_kernel<BITS, 1, false, ST, OUTC>), grid, block, lds, stream, a);
  else if (a.w.mid_side)
    AAD_LAUNCH((decode_window_channel_mix_kernel<BITS, 2, true, ST, OUTC>), grid, block, lds, stream, a);
  else
    AAD_LAUNCH((decode_window_channel_mix_kernel<BITS, 2, false, ST, OUTC>), grid, block, lds, stream, a);
}

template <int ST, int OUTC>
static void launch_type(const ChannelMixWindowArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.w.bits == 4) launch_bits<4, ST, OUTC>(a, grid, block, lds, stream);
  else if (a.w.bits == 3) launch_bits<3, ST, OUTC>(a, grid, block, lds, stream);
  else launch_bits<2, ST, OUTC>(a, grid, block, lds, stream);
}

/* one launch of a run: a.w.channels / a.w.bits / a.w.mid_side name the variant, a.out_channels (1 or 2) the output */
template <>
void launch_decode_window_channel_mix_unit<AAD_WINDOW_HALF != 0>(
    const ChannelMixWindowArgs &a, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  using T = WindowUnitTypes<AAD_WINDOW_HALF != 0>;
  const dim3 grid(p.grid), block(p.workgroup);
  if (a.out_channels == 1) {
    if (sample_type == T::second) launch_type<T::second, 1>(a, grid, block, p.lds, stream);
    else launch_type<T::first, 1>(a, grid, block, p.lds, stream);
  } else {
    if (sample_type == T::second) launch_type<T::second, 2>(a, grid, block, p.lds, stream);
    else launch_type<T::first, 2>(a, grid, block, p.lds, stream);
  }
}

} /* namespace aad */
