/* aad_decode_window_gain.hip - translation unit of the same-format window decoder with a per-window gain
 * (aad_decode_window_gain.hip.h).  AAD_WINDOW_HALF=0: float32 rows alone (a gain has no int16 rows). */
#include "aad_decode_window_gain.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::Same, WindowMode::Gain> {
  using Args = WindowGainArgs;
  static Args pack(const WindowUnitRun &r) { return Args{r.w, r.gain, r.add, 0}; }
  static const WindowArgs &window(const Args &a) { return a.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_gain_kernel<BITS, CHF, MS, ST>;
};
AAD_WINDOW_UNIT(Same, Gain);

} /* namespace aad */
