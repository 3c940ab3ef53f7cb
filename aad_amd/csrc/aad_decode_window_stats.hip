/* aad_decode_window_stats.hip - translation unit of the same-format window decoder with statistics
 * (aad_decode_window_stats.hip.h). */
#include "aad_decode_window_stats.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Same, WindowMode::Stats> {
  using Args = WindowStatsArgs;
  static Args pack(const WindowUnitRun &r) { return Args{r.w, stats_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_stats_kernel<BITS, CHF, MS, ST>;
};
AAD_WINDOW_UNIT(Same, Stats);

} /* namespace aad */
