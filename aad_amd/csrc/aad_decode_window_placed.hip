/* aad_decode_window_placed.hip - translation unit of the same-format window decoder with a span per window
 * (aad_decode_window_placed.hip.h).  AAD_WINDOW_HALF=0: float32 rows alone. */
#include "aad_decode_window_placed.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Same, WindowMode::Placed> {
  using Args = WindowPlacedArgs;
  static Args pack(const WindowUnitRun &r) { return Args{{r.w, r.gain, r.add, 0}, span_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.g.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_placed_kernel<BITS, CHF, MS, ST>;
};
AAD_WINDOW_UNIT(Same, Placed);

} /* namespace aad */
