/* aad_decode_window_placed_stats.hip - translation unit of the same-format window decoder's statistics over a span per window
 * (aad_decode_window_placed.hip.h).  No rows, so one object: AAD_WINDOW_HALF does not apply. */
#include "aad_decode_window_placed.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Same, WindowMode::PlacedStats> {
  using Args = WindowPlacedStatsArgs;
  static Args pack(const WindowUnitRun &r) { return Args{{r.w, stats_words(r)}, span_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.s.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_placed_stats_kernel<BITS, CHF, MS>;
};
AAD_WINDOW_UNIT(Same, PlacedStats);

} /* namespace aad */
