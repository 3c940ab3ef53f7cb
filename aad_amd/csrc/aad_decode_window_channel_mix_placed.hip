/* aad_decode_window_channel_mix_placed.hip - translation unit of the channel-mix window decoder with a span per window
 * (aad_decode_window_placed.hip.h).  AAD_WINDOW_HALF=0: float32 rows alone. */
#include "aad_decode_window_placed.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::ChannelMix, WindowMode::Placed> {
  using Args = ChannelMixWindowPlacedArgs;
  static Args pack(const WindowUnitRun &r) { return Args{{channel_mix_window_args(r), r.gain, r.add, 0}, span_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.g.m.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_channel_mix_placed_kernel<BITS, CHF, MS, ST, OUTC>;
};
AAD_WINDOW_UNIT(ChannelMix, Placed);

} /* namespace aad */
