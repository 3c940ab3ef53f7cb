/* aad_decode_window_stats.hip - translation unit of the same-format window decoder with statistics
 * (aad_decode_window_stats.hip.h). */
#include "aad_decode_window_stats.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS, int ST>
static void launch_bits(const WindowStatsArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.w.channels == 1)
    AAD_LAUNCH((decode_window_stats_kernel<BITS, 1, false, ST>), grid, block, lds, stream, a);
  else if (a.w.channels == 2 && a.w.mid_side)
    AAD_LAUNCH((decode_window_stats_kernel<BITS, 2, true, ST>), grid, block, lds, stream, a);
  else if (a.w.channels == 2)
    AAD_LAUNCH((decode_window_stats_kernel<BITS, 2, false, ST>), grid, block, lds, stream, a);
  else
    AAD_LAUNCH((decode_window_stats_kernel<BITS, 0, false, ST>), grid, block, lds, stream, a);
}

template <int ST>
static void launch_type(const WindowStatsArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.w.bits == 4) launch_bits<4, ST>(a, grid, block, lds, stream);
  else if (a.w.bits == 3) launch_bits<3, ST>(a, grid, block, lds, stream);
  else launch_bits<2, ST>(a, grid, block, lds, stream);
}

template <>
void launch_decode_window_stats_unit<AAD_WINDOW_HALF != 0>(
    const WindowArgs &args, struct AADHipRowStats *stats, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  const WindowStatsArgs a = {args, reinterpret_cast<unsigned long long *>(stats)};
  using T = WindowUnitTypes<AAD_WINDOW_HALF != 0>;
  const dim3 grid(p.grid), block(p.workgroup);
  if (sample_type == T::second) launch_type<T::second>(a, grid, block, p.lds, stream);
  else launch_type<T::first>(a, grid, block, p.lds, stream);
}

} /* namespace aad */
