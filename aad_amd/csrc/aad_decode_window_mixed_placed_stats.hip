/* aad_decode_window_mixed_placed_stats.hip - translation unit of the mixed-format window decoder's statistics over a span per
 * window (aad_decode_window_placed.hip.h).  No rows, so one object: AAD_WINDOW_HALF does not apply. */
#include "aad_decode_window_placed.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Mixed, WindowMode::PlacedStats> {
  using Args = MixedWindowPlacedStatsArgs;
  static Args pack(const WindowUnitRun &r) { return Args{{mixed_window_args(r), stats_words(r)}, span_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.s.m.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_mixed_placed_stats_kernel<BITS, CHF, MS>;
};
AAD_WINDOW_UNIT(Mixed, PlacedStats);

} /* namespace aad */
