/* aad_decode_window_mixed.hip - translation unit of the mixed-format window decoder (aad_decode_window_mixed.hip.h). */
#include "aad_decode_window_mixed.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Mixed, WindowMode::Rows> {
  using Args = MixedWindowArgs;
  static Args pack(const WindowUnitRun &r) { return mixed_window_args(r); }
  static const WindowArgs &window(const Args &a) { return a.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_mixed_kernel<BITS, CHF, MS, ST>;
};
AAD_WINDOW_UNIT(Mixed, Rows);

} /* namespace aad */
