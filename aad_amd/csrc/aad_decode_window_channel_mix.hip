/* aad_decode_window_channel_mix.hip - translation unit of the channel-mix window decoder (aad_decode_window_channel_mix.hip.h).
 * */
#include "aad_decode_window_channel_mix.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::ChannelMix, WindowMode::Rows> {
  using Args = ChannelMixWindowArgs;
  static Args pack(const WindowUnitRun &r) { return channel_mix_window_args(r); }
  static const WindowArgs &window(const Args &a) { return a.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_channel_mix_kernel<BITS, CHF, MS, ST, OUTC>;
};
AAD_WINDOW_UNIT(ChannelMix, Rows);

} /* namespace aad */
