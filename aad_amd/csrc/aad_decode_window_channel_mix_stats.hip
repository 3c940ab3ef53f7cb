/* aad_decode_window_channel_mix_stats.hip - translation unit of the channel-mix window decoder with statistics
 * (aad_decode_window_stats.hip.h). */
#include "aad_decode_window_stats.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS, bool F32, int OUTC>
static void launch_bits(const ChannelMixWindowStatsArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.m.w.channels == 1)
    AAD_LAUNCH((decode_window_channel_mix_stats_kernel<BITS, 1, false, F32, OUTC>), grid, block, lds, stream, a);
  else if (a.m.w.mid_side)
    AAD_LAUNCH((decode_window_channel_mix_stats_kernel<BITS, 2, true, F32, OUTC>), grid, block, lds, stream, a);
  else
    AAD_LAUNCH((decode_window_channel_mix_stats_kernel<BITS, 2, false, F32, OUTC>), grid, block, lds, stream, a);
}

template <bool F32, int OUTC>
static void launch_type(const ChannelMixWindowStatsArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.m.w.bits == 4) launch_bits<4, F32, OUTC>(a, grid, block, lds, stream);
  else if (a.m.w.bits == 3) launch_bits<3, F32, OUTC>(a, grid, block, lds, stream);
  else launch_bits<2, F32, OUTC>(a, grid, block, lds, stream);
}

/* one launch of a run: args.w.channels / args.w.bits / args.w.mid_side name the variant, args.out_channels (1 or 2) the output */
void launch_decode_window_channel_mix_stats(const ChannelMixWindowArgs &args, struct AADHipRowStats *stats, const WindowLaunch &p,
                                            bool float32, hipStream_t stream)
{
  const ChannelMixWindowStatsArgs a = {args, reinterpret_cast<unsigned long long *>(stats)};
  const dim3 grid(p.grid), block(p.workgroup);
  if (args.out_channels == 1) {
    if (float32) launch_type<true, 1>(a, grid, block, p.lds, stream);
    else launch_type<false, 1>(a, grid, block, p.lds, stream);
  } else {
    if (float32) launch_type<true, 2>(a, grid, block, p.lds, stream);
    else launch_type<false, 2>(a, grid, block, p.lds, stream);
  }
}

} /* namespace aad */
