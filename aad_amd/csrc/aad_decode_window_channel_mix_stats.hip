/* aad_decode_window_channel_mix_stats.hip - translation unit of the channel-mix window decoder with statistics
 * (aad_decode_window_stats.hip.h). */
#include "aad_decode_window_stats.hip.h"
#include "aad_window_unit.hip.h"

namespace aad {

template <>
struct WindowUnit<WindowKind::ChannelMix, WindowMode::Stats> {
  using Args = ChannelMixWindowStatsArgs;
  static Args pack(const WindowUnitRun &r) { return Args{channel_mix_window_args(r), stats_words(r)}; }
  static const WindowArgs &window(const Args &a) { return a.m.w; }
  template <int BITS, int CHF, bool MS, int ST, int OUTC>
  static constexpr auto kernel = &decode_window_channel_mix_stats_kernel<BITS, CHF, MS, ST, OUTC>;
};
AAD_WINDOW_UNIT(ChannelMix, Stats);

} /* namespace aad */
