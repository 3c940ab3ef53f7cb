/* aad_decode_window_channel_mix_placed_stats.hip - translation unit of the channel-mix window decoder's statistics over a span
 * per window (aad_decode_window_placed.hip.h).  No rows, so one object: AAD_WINDOW_HALF does not apply. */
#include "aad_decode_window_placed.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS, int OUTC>
static void launch_bits(const ChannelMixWindowPlacedStatsArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.s.m.w.channels == 1)
    AAD_LAUNCH((decode_window_channel_mix_placed_stats_kernel<BITS, 1, false, OUTC>), grid, block, lds, stream, a);
  else if (a.s.m.w.mid_side)
    AAD_LAUNCH((decode_window_channel_mix_placed_stats_kernel<BITS, 2, true, OUTC>), grid, block, lds, stream, a);
  else
    AAD_LAUNCH((decode_window_channel_mix_placed_stats_kernel<BITS, 2, false, OUTC>), grid, block, lds, stream, a);
}

template <int OUTC>
static void launch_rows(const ChannelMixWindowPlacedStatsArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.s.m.w.bits == 4) launch_bits<4, OUTC>(a, grid, block, lds, stream);
  else if (a.s.m.w.bits == 3) launch_bits<3, OUTC>(a, grid, block, lds, stream);
  else launch_bits<2, OUTC>(a, grid, block, lds, stream);
}

/* one launch of a run: args.w.channels / args.w.bits / args.w.mid_side name the variant, args.out_channels (1 or 2) the output */
void launch_decode_window_channel_mix_placed_stats(const ChannelMixWindowArgs &args, const struct AADHipWindowSpan *spans,
                                                   struct AADHipRowStats *stats, const WindowLaunch &p, hipStream_t stream)
{
  const ChannelMixWindowPlacedStatsArgs a = {{args, reinterpret_cast<unsigned long long *>(stats)},
                                             reinterpret_cast<const uint64_t *>(spans)};
  const dim3 grid(p.grid), block(p.workgroup);
  if (a.s.m.out_channels == 1) launch_rows<1>(a, grid, block, p.lds, stream);
  else launch_rows<2>(a, grid, block, p.lds, stream);
}

} /* namespace aad */
