/* aad_decode_window_mixed_stats.hip - translation unit of the mixed-format window decoder with statistics
 * (aad_decode_window_stats.hip.h). */
#include "aad_decode_window_stats.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Mixed, WindowMode::Stats> {
  using Args = MixedWindowStatsArgs;
  static Args pack(const WindowUnitRun &r) { return Args{mixed_window_args(r), stats_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.m.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_mixed_stats_kernel<BITS, CHF, MS, ST>;
};
AAD_WINDOW_UNIT(Mixed, Stats);

} /* namespace aad */
