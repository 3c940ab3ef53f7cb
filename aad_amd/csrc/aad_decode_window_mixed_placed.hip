/* aad_decode_window_mixed_placed.hip - translation unit of the mixed-format window decoder with a span per window
 * (aad_decode_window_placed.hip.h).  AAD_WINDOW_HALF=0: float32 rows alone. */
#include "aad_decode_window_placed.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Mixed, WindowMode::Placed> {
  using Args = MixedWindowPlacedArgs;
  static Args pack(const WindowUnitRun &r) { return Args{{mixed_window_args(r), r.gain, r.add, 0}, span_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.g.m.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_mixed_placed_kernel<BITS, CHF, MS, ST>;
};
AAD_WINDOW_UNIT(Mixed, Placed);

} /* namespace aad */
