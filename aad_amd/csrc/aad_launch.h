/*
 * aad_launch.h - kernel launches that can carry a completion event on their own dispatch packet.
 *
 * AADHip_ContextSignalNextRun (include/aad_hip.h) asks for events to be recorded when a plan run's work starts / is done.  Every
 * plan run is ONE kernel, so the events ride on that kernel's dispatch (hipExtLaunchKernelGGL's start / stop event) instead of on
 * barrier packets of their own around it: measured on MI355X (tools/microbench/ubench_event_gap.hip,
 * profiles/r03_microbench_event_gap.txt) a hipEventRecord behind every kernel of a back-to-back sequence costs the queue
 * 2.9 us per launch, the attached event nothing.  The events travel from the entry point to the launch site in a
 * thread-local (the launch helpers are templates several levels down); the first AAD_LAUNCH of the thread takes them.
 */
#ifndef AAD_LAUNCH_H_INCLUDED
#define AAD_LAUNCH_H_INCLUDED

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "aad_launch_policy.h"

namespace aad {
struct LaunchSignal {
  hipEvent_t start, stop; /* either may be null */
};
extern thread_local LaunchSignal tl_launch_signal; /* defined in aad_hip_engine.hip; both null when no run asked for events */

/* The decoders with translation units of their own, launched as planned (aad_launch_policy.h).  aad_decode_split.hip is compiled
 * with its own instruction-scheduling strategy (see the Makefile); the residual rows of DecodeKernel::SplitScratch go through
 * `residual` (p.residual_bytes of device memory).  aad_decode_tiled.hip: DecodeKernel::Tiled. */
struct DecodeArgs;
void launch_decode_split(const DecodeArgs &args, const DecodeLaunch &p, int32_t *residual, hipStream_t stream);
void launch_decode_tiled(const DecodeArgs &args, const DecodeLaunch &p, hipStream_t stream);
/* The window decoders (AADHip_WindowDecodePlanRun, ...RunStats, ...RunGain, ...RunPlaced).  Each of their twelve translation units
 * that write rows is compiled twice (Makefile): with AAD_WINDOW_HALF=0 its kernels write int16 and float32 rows, with AAD_WINDOW_HALF=1 (the _half
 * objects) float16 and bfloat16 rows.  A unit defines launch_..._unit<AAD_WINDOW_HALF>; the launch_... below pick the unit by the
 * run's sample_type (enum AADHipSampleType, validated by the entry point). */
#ifndef AAD_WINDOW_HALF
#define AAD_WINDOW_HALF 0
#endif
template <bool HALF>
struct WindowUnitTypes { /* a unit's two sample types: sample_type == second runs the second, anything else the first */
  static constexpr int32_t first = HALF ? AAD_HIP_SAMPLE_FLOAT16 : AAD_HIP_SAMPLE_INT16;
  static constexpr int32_t second = HALF ? AAD_HIP_SAMPLE_BFLOAT16 : AAD_HIP_SAMPLE_FLOAT32;
};
/* the unit's launch function: declared with both explicit specialisations, one defined by each object of the unit */
#define AAD_WINDOW_UNIT(name, ...)     \
  template <bool HALF>                 \
  void name(__VA_ARGS__);              \
  template <>                          \
  void name<false>(__VA_ARGS__);       \
  template <>                          \
  void name<true>(__VA_ARGS__)
inline bool window_half_type(int32_t sample_type)
{
  return sample_type == AAD_HIP_SAMPLE_FLOAT16 || sample_type == AAD_HIP_SAMPLE_BFLOAT16;
}
/* aad_decode_window.hip: the same-format window decoder */
struct WindowArgs;
AAD_WINDOW_UNIT(launch_decode_window_unit,
                const WindowArgs &args, const WindowLaunch &p, int32_t sample_type, hipStream_t stream);
/* aad_decode_window_mixed.hip: one launch (one kernel variant: args.w.bits, args.w.mid_side) of a mixed-format window decode run */
struct MixedWindowArgs;
AAD_WINDOW_UNIT(launch_decode_window_mixed_unit,
                const MixedWindowArgs &args, const WindowLaunch &p, int32_t sample_type, hipStream_t stream);
/* aad_decode_window_channel_mix.hip: one launch (args.w.channels, args.w.bits, args.w.mid_side: the variant) of a channel-mix run */
struct ChannelMixWindowArgs;
AAD_WINDOW_UNIT(launch_decode_window_channel_mix_unit,
                const ChannelMixWindowArgs &args, const WindowLaunch &p, int32_t sample_type, hipStream_t stream);
/* aad_decode_window_stats.hip, aad_decode_window_mixed_stats.hip, aad_decode_window_channel_mix_stats.hip: the same launches of
 * AADHip_WindowDecodePlanRunStats - the rows (args' out, which may be null) and the level statistics of every row added into
 * `stats`, which the run cleared */
AAD_WINDOW_UNIT(launch_decode_window_stats_unit,
                const WindowArgs &args, struct AADHipRowStats *stats, const WindowLaunch &p, int32_t sample_type,
                hipStream_t stream);
AAD_WINDOW_UNIT(launch_decode_window_mixed_stats_unit,
                const MixedWindowArgs &args, struct AADHipRowStats *stats, const WindowLaunch &p, int32_t sample_type,
                hipStream_t stream);
AAD_WINDOW_UNIT(launch_decode_window_channel_mix_stats_unit,
                const ChannelMixWindowArgs &args, struct AADHipRowStats *stats, const WindowLaunch &p, int32_t sample_type,
                hipStream_t stream);
/* aad_decode_window_gain.hip, aad_decode_window_mixed_gain.hip, aad_decode_window_channel_mix_gain.hip: the same launches of
 * AADHip_WindowDecodePlanRunGain - float rows scaled by the window's gain (`gain`: device memory, null for 1) and stored, or with
 * `add` added to what the rows hold.  Their AAD_WINDOW_HALF=0 objects hold float32 alone */
AAD_WINDOW_UNIT(launch_decode_window_gain_unit,
                const WindowArgs &args, const float *gain, uint32_t add, const WindowLaunch &p, int32_t sample_type,
                hipStream_t stream);
AAD_WINDOW_UNIT(launch_decode_window_mixed_gain_unit,
                const MixedWindowArgs &args, const float *gain, uint32_t add, const WindowLaunch &p, int32_t sample_type,
                hipStream_t stream);
AAD_WINDOW_UNIT(launch_decode_window_channel_mix_gain_unit,
                const ChannelMixWindowArgs &args, const float *gain, uint32_t add, const WindowLaunch &p, int32_t sample_type,
                hipStream_t stream);
/* aad_decode_window_placed.hip, aad_decode_window_mixed_placed.hip, aad_decode_window_channel_mix_placed.hip: the same launches of
 * AADHip_WindowDecodePlanRunPlaced - the gain units' rows, each window's crop clipped to and placed by its record of `spans`
 * (device memory, null: every span is (T, 0)).  Compiled twice as the gain units are */
AAD_WINDOW_UNIT(launch_decode_window_placed_unit,
                const WindowArgs &args, const struct AADHipWindowSpan *spans, const float *gain, uint32_t add, const WindowLaunch &p,
                int32_t sample_type, hipStream_t stream);
AAD_WINDOW_UNIT(launch_decode_window_mixed_placed_unit,
                const MixedWindowArgs &args, const struct AADHipWindowSpan *spans, const float *gain, uint32_t add,
                const WindowLaunch &p, int32_t sample_type, hipStream_t stream);
AAD_WINDOW_UNIT(launch_decode_window_channel_mix_placed_unit,
                const ChannelMixWindowArgs &args, const struct AADHipWindowSpan *spans, const float *gain, uint32_t add,
                const WindowLaunch &p, int32_t sample_type, hipStream_t stream);
/* aad_decode_window_placed_stats.hip, aad_decode_window_mixed_placed_stats.hip, aad_decode_window_channel_mix_placed_stats.hip: the
 * same launches of AADHip_WindowDecodePlanRunPlacedStats - the level statistics of every window's clipped crop added into `stats`,
 * which the run cleared; no rows (args' out is null), so no sample type and one object each */
void launch_decode_window_placed_stats(const WindowArgs &args, const struct AADHipWindowSpan *spans, struct AADHipRowStats *stats,
                                       const WindowLaunch &p, hipStream_t stream);
void launch_decode_window_mixed_placed_stats(const MixedWindowArgs &args, const struct AADHipWindowSpan *spans,
                                             struct AADHipRowStats *stats, const WindowLaunch &p, hipStream_t stream);
void launch_decode_window_channel_mix_placed_stats(const ChannelMixWindowArgs &args, const struct AADHipWindowSpan *spans,
                                                   struct AADHipRowStats *stats, const WindowLaunch &p, hipStream_t stream);

inline void launch_decode_window_placed(const WindowArgs &args, const struct AADHipWindowSpan *spans, const float *gain, uint32_t add,
                                        const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_placed_unit<true>(args, spans, gain, add, p, sample_type, stream);
  else launch_decode_window_placed_unit<false>(args, spans, gain, add, p, sample_type, stream);
}
inline void launch_decode_window_mixed_placed(const MixedWindowArgs &args, const struct AADHipWindowSpan *spans, const float *gain,
                                              uint32_t add, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_mixed_placed_unit<true>(args, spans, gain, add, p, sample_type, stream);
  else launch_decode_window_mixed_placed_unit<false>(args, spans, gain, add, p, sample_type, stream);
}
inline void launch_decode_window_channel_mix_placed(const ChannelMixWindowArgs &args, const struct AADHipWindowSpan *spans,
                                                    const float *gain, uint32_t add, const WindowLaunch &p, int32_t sample_type,
                                                    hipStream_t stream)
{
  if (window_half_type(sample_type))
    launch_decode_window_channel_mix_placed_unit<true>(args, spans, gain, add, p, sample_type, stream);
  else launch_decode_window_channel_mix_placed_unit<false>(args, spans, gain, add, p, sample_type, stream);
}

inline void launch_decode_window(const WindowArgs &args, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_unit<true>(args, p, sample_type, stream);
  else launch_decode_window_unit<false>(args, p, sample_type, stream);
}
inline void launch_decode_window_mixed(const MixedWindowArgs &args, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_mixed_unit<true>(args, p, sample_type, stream);
  else launch_decode_window_mixed_unit<false>(args, p, sample_type, stream);
}
inline void launch_decode_window_channel_mix(const ChannelMixWindowArgs &args, const WindowLaunch &p, int32_t sample_type,
                                             hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_channel_mix_unit<true>(args, p, sample_type, stream);
  else launch_decode_window_channel_mix_unit<false>(args, p, sample_type, stream);
}
inline void launch_decode_window_stats(const WindowArgs &args, struct AADHipRowStats *stats, const WindowLaunch &p,
                                       int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_stats_unit<true>(args, stats, p, sample_type, stream);
  else launch_decode_window_stats_unit<false>(args, stats, p, sample_type, stream);
}
inline void launch_decode_window_mixed_stats(const MixedWindowArgs &args, struct AADHipRowStats *stats, const WindowLaunch &p,
                                             int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_mixed_stats_unit<true>(args, stats, p, sample_type, stream);
  else launch_decode_window_mixed_stats_unit<false>(args, stats, p, sample_type, stream);
}
inline void launch_decode_window_channel_mix_stats(const ChannelMixWindowArgs &args, struct AADHipRowStats *stats,
                                                   const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_channel_mix_stats_unit<true>(args, stats, p, sample_type, stream);
  else launch_decode_window_channel_mix_stats_unit<false>(args, stats, p, sample_type, stream);
}
inline void launch_decode_window_gain(const WindowArgs &args, const float *gain, uint32_t add, const WindowLaunch &p,
                                      int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_gain_unit<true>(args, gain, add, p, sample_type, stream);
  else launch_decode_window_gain_unit<false>(args, gain, add, p, sample_type, stream);
}
inline void launch_decode_window_mixed_gain(const MixedWindowArgs &args, const float *gain, uint32_t add, const WindowLaunch &p,
                                            int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_mixed_gain_unit<true>(args, gain, add, p, sample_type, stream);
  else launch_decode_window_mixed_gain_unit<false>(args, gain, add, p, sample_type, stream);
}
inline void launch_decode_window_channel_mix_gain(const ChannelMixWindowArgs &args, const float *gain, uint32_t add,
                                                  const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  if (window_half_type(sample_type)) launch_decode_window_channel_mix_gain_unit<true>(args, gain, add, p, sample_type, stream);
  else launch_decode_window_channel_mix_gain_unit<false>(args, gain, add, p, sample_type, stream);
}
/* the decoded rows of a planar reconstruct run (AADHip_PlanarReconstructPlanRun; launched through aad_encode_launch.hip.h).
 * base: per stream (segmented: per chain) the element of `out` that holds channel 0's sample of the lane's first frame, device
 * memory */
struct RecRows {
  void *out;
  const uint64_t *base;
  uint64_t channel_stride;
};
}

#define AAD_LAUNCH(kernel, grid, block, lds, stream, ...)                                                           \
  do {                                                                                                              \
    const aad::LaunchSignal aad_signal_ = aad::tl_launch_signal;                                                    \
    aad::tl_launch_signal = aad::LaunchSignal{nullptr, nullptr};                                                    \
    if (aad_signal_.start != nullptr || aad_signal_.stop != nullptr)                                                \
      hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, aad_signal_.start, aad_signal_.stop, 0, __VA_ARGS__); \
    else                                                                                                            \
      hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                            \
  } while (0)

#endif /* AAD_LAUNCH_H_INCLUDED */
