/* aad_decode_window.hip - translation unit of the window decoder (aad_decode_window.hip.h). */
#include "aad_decode_window.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Same, WindowMode::Rows> {
  using Args = WindowArgs;
  static Args pack(const WindowUnitRun &r) { return r.w; }
  static const WindowArgs &window(const Args &a) { return a; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_kernel<BITS, CHF, MS, ST>;
};
AAD_WINDOW_UNIT(Same, Rows);

} /* namespace aad */
