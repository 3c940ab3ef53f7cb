/* aad_decode_window_mixed_placed_stats.hip - translation unit of the mixed-format window decoder's statistics over a span per
 * window (aad_decode_window_placed.hip.h).  No rows, so one object: AAD_WINDOW_HALF does not apply. */
#include "aad_decode_window_placed.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS>
static void launch_bits(const MixedWindowPlacedStatsArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.s.m.w.channels == 1)
    AAD_LAUNCH((decode_window_mixed_placed_stats_kernel<BITS, 1, false>), grid, block, lds, stream, a);
  else if (a.s.m.w.channels == 2 && a.s.m.w.mid_side)
    AAD_LAUNCH((decode_window_mixed_placed_stats_kernel<BITS, 2, true>), grid, block, lds, stream, a);
  else if (a.s.m.w.channels == 2)
    AAD_LAUNCH((decode_window_mixed_placed_stats_kernel<BITS, 2, false>), grid, block, lds, stream, a);
  else
    AAD_LAUNCH((decode_window_mixed_placed_stats_kernel<BITS, 0, false>), grid, block, lds, stream, a);
}

/* one launch of a run: args.w.bits / args.w.mid_side name the variant */
void launch_decode_window_mixed_placed_stats(const MixedWindowArgs &args, const struct AADHipWindowSpan *spans,
                                             struct AADHipRowStats *stats, const WindowLaunch &p, hipStream_t stream)
{
  const MixedWindowPlacedStatsArgs a = {{args, reinterpret_cast<unsigned long long *>(stats)},
                                        reinterpret_cast<const uint64_t *>(spans)};
  const dim3 grid(p.grid), block(p.workgroup);
  if (a.s.m.w.bits == 4) launch_bits<4>(a, grid, block, p.lds, stream);
  else if (a.s.m.w.bits == 3) launch_bits<3>(a, grid, block, p.lds, stream);
  else launch_bits<2>(a, grid, block, p.lds, stream);
}

} /* namespace aad */
