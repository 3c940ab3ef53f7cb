/*
 * aad_window_unit.hip.h - the launch nest of the window decode units: from one launch of a run (aad_launch.h WindowUnitRun) to the
 * kernel instantiation that decodes it.  Every unit runs window_lane (aad_decode_window.hip.h) under a kernel and an argument
 * struct of its own; it describes them in a specialisation of WindowUnit<KIND, MODE>
 *   using Args                                    the kernel's argument struct
 *   static Args pack(const WindowUnitRun &r)      ... filled from the launch
 *   static const WindowArgs &window(const Args &) ... and the WindowArgs inside it
 *   template <int BITS, int CHF, bool MS, int ST, int OUTC> static constexpr auto kernel
 *                                                 the kernel's address (ST, OUTC: where the kernel template has them)
 * and names itself with AAD_WINDOW_UNIT(KIND, MODE), which instantiates launch_window_object for the object being compiled.
 * Which kernels an object holds follows from the nest alone: bits 4 / 3 / 2, channels 1 / 2 with mid/side / 2 / any other count
 * (CHF 0; a channel-mix source is mono or stereo, and its units add out_channels 1 / 2), and the object's row types.
 */
#ifndef AAD_WINDOW_UNIT_HIP_H
#define AAD_WINDOW_UNIT_HIP_H

#include "aad_decode_window_channel_mix.hip.h"
#include "aad_decode_window_mixed.hip.h"
#include "aad_launch.h"

namespace aad {

template <WindowKind KIND, WindowMode MODE>
struct WindowUnit;

/* what the mixed-format and channel-mix kernels' argument structs start with */
inline MixedWindowArgs mixed_window_args(const WindowUnitRun &r)
{
  return MixedWindowArgs{r.w, static_cast<const StreamFormat *>(r.formats), r.owns_strays, 0};
}
inline ChannelMixWindowArgs channel_mix_window_args(const WindowUnitRun &r)
{
  return ChannelMixWindowArgs{r.w, static_cast<const ChannelStreamFormat *>(r.formats), r.owns_strays, r.out_channels};
}

/* the tables of a run as the kernels take them */
inline unsigned long long *stats_words(const WindowUnitRun &r) { return reinterpret_cast<unsigned long long *>(r.stats); }
inline const uint64_t *span_words(const WindowUnitRun &r) { return reinterpret_cast<const uint64_t *>(r.spans); }

/* an object's row types: sample_type == second runs the second, anything else the first.  A gain has no int16 rows, and the
 * statistics of placed windows are those of int16 rows that are not there */
template <WindowMode MODE, bool HALF>
struct WindowUnitTypes {
  static constexpr int32_t first = HALF                                                      ? AAD_HIP_SAMPLE_FLOAT16
                                   : MODE == WindowMode::Gain || MODE == WindowMode::Placed ? AAD_HIP_SAMPLE_FLOAT32
                                                                                              : AAD_HIP_SAMPLE_INT16;
  static constexpr int32_t second = HALF                             ? AAD_HIP_SAMPLE_BFLOAT16
                                    : MODE == WindowMode::PlacedStats ? first
                                                                      : AAD_HIP_SAMPLE_FLOAT32;
};

template <class U, bool MIX, int ST, int OUTC, int BITS>
void launch_window_channels(const typename U::Args &a, const WindowLaunch &p, hipStream_t stream)
{
  const WindowArgs &w = U::window(a);
  const dim3 grid(p.grid), block(p.workgroup);
  const bool two = MIX || w.channels == 2;
  if (w.channels == 1) AAD_LAUNCH((U::template kernel<BITS, 1, false, ST, OUTC>), grid, block, p.lds, stream, a);
  else if (two && w.mid_side) AAD_LAUNCH((U::template kernel<BITS, 2, true, ST, OUTC>), grid, block, p.lds, stream, a);
  else if (two) AAD_LAUNCH((U::template kernel<BITS, 2, false, ST, OUTC>), grid, block, p.lds, stream, a);
  else if constexpr (!MIX) AAD_LAUNCH((U::template kernel<BITS, 0, false, ST, OUTC>), grid, block, p.lds, stream, a);
}

template <class U, bool MIX, int ST, int OUTC>
void launch_window_bits(const typename U::Args &a, const WindowLaunch &p, hipStream_t stream)
{
  const uint32_t bits = U::window(a).bits;
  if (bits == 4) launch_window_channels<U, MIX, ST, OUTC, 4>(a, p, stream);
  else if (bits == 3) launch_window_channels<U, MIX, ST, OUTC, 3>(a, p, stream);
  else launch_window_channels<U, MIX, ST, OUTC, 2>(a, p, stream);
}

/* the rows of a window, out_channels: a channel-mix unit's kernels have them as a template parameter */
template <class U, bool MIX, int ST>
void launch_window_out(const typename U::Args &a, uint32_t out_channels, const WindowLaunch &p, hipStream_t stream)
{
  if constexpr (!MIX) launch_window_bits<U, false, ST, 0>(a, p, stream);
  else if (out_channels == 1) launch_window_bits<U, true, ST, 1>(a, p, stream);
  else launch_window_bits<U, true, ST, 2>(a, p, stream);
}

/* The order of the nest is the order the kernels are instantiated in, which is their order in the object's code, and a kernel's
 * bytes depend on its place there (it reaches its tables pc-relative).  The channel-mix row and statistics objects have always
 * picked out_channels in front of the row type and every other object the type first: both orders stay, so that no kernel moves. */
template <WindowKind KIND, WindowMode MODE, bool HALF>
void launch_window_object(const WindowUnitRun &r, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  using U = WindowUnit<KIND, MODE>;
  using T = WindowUnitTypes<MODE, HALF>;
  constexpr bool MIX = KIND == WindowKind::ChannelMix;
  const typename U::Args a = U::pack(r);
  if constexpr (MIX && (MODE == WindowMode::Rows || MODE == WindowMode::Stats)) {
    const bool second = sample_type == T::second;
    if (r.out_channels == 1 && second) launch_window_bits<U, true, T::second, 1>(a, p, stream);
    else if (r.out_channels == 1) launch_window_bits<U, true, T::first, 1>(a, p, stream);
    else if (second) launch_window_bits<U, true, T::second, 2>(a, p, stream);
    else launch_window_bits<U, true, T::first, 2>(a, p, stream);
  } else {
    if constexpr (T::second != T::first)
      if (sample_type == T::second) return launch_window_out<U, MIX, T::second>(a, r.out_channels, p, stream);
    launch_window_out<U, MIX, T::first>(a, r.out_channels, p, stream);
  }
}

#define AAD_WINDOW_UNIT(KIND, MODE)                                                          \
  template void launch_window_object<WindowKind::KIND, WindowMode::MODE, AAD_WINDOW_HALF != 0>( \
      const WindowUnitRun &, const WindowLaunch &, int32_t, hipStream_t)

} /* namespace aad */

#endif /* AAD_WINDOW_UNIT_HIP_H */
