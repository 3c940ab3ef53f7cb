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
extern thread_local LaunchSignal tl_launch_signal; /* defined in aad_hip_engine.hip, whose plan runs set it (the FIR stages of
                                                    * aad_fir_stage.hip never do); both null when no run asked for events */

/* The decoders with translation units of their own, launched as planned (aad_launch_policy.h).  aad_decode_split.hip is compiled
 * with its own instruction-scheduling strategy (see the Makefile); the residual rows of DecodeKernel::SplitScratch go through
 * `residual` (p.residual_bytes of device memory).  aad_decode_tiled.hip: DecodeKernel::Tiled. */
struct DecodeArgs;
void launch_decode_split(const DecodeArgs &args, const DecodeLaunch &p, int32_t *residual, hipStream_t stream);
void launch_decode_tiled(const DecodeArgs &args, const DecodeLaunch &p, hipStream_t stream);
/* The window decoders (AADHip_WindowDecodePlanRun, ...RunStats, ...RunGain, ...RunPlaced, ...RunPlacedStats): one translation unit
 * per plan kind (aad_launch_policy.h WindowKind) and mode, aad_decode_window[_mixed|_channel_mix][_stats|_gain|_placed|_placed_stats].hip.
 * Each of the twelve that write rows is compiled twice (Makefile): with AAD_WINDOW_HALF=0 its kernels write int16 and float32 rows -
 * the gain and placed units float32 alone - and with AAD_WINDOW_HALF=1 (the _half objects) float16 and bfloat16 rows.  The
 * placed-stats units write no rows: one object each, and no sample type. */
#ifndef AAD_WINDOW_HALF
#define AAD_WINDOW_HALF 0
#endif
enum class WindowMode { Rows, Stats, Gain, Placed, PlacedStats };
inline bool window_half_type(int32_t sample_type)
{
  return sample_type == AAD_HIP_SAMPLE_FLOAT16 || sample_type == AAD_HIP_SAMPLE_BFLOAT16;
}
/* One launch of a run, as every unit takes it: the unit packs what its kernel's argument struct holds of this.
 * w.channels / w.bits / w.mid_side name the launch's kernel variant, out_channels (1 or 2, a channel-mix run's) the rows */
struct WindowArgs;
struct WindowUnitRun {
  const WindowArgs &w;
  const void *formats;  /* Mixed: StreamFormat, ChannelMix: ChannelStreamFormat, [w.num_streams] in device memory; Same: unused */
  uint32_t owns_strays; /* Mixed, ChannelMix: this launch writes the windows whose stream is out of range */
  uint32_t out_channels; /* ChannelMix */
  const float *gain;    /* Gain, Placed: float rows scaled by the window's gain (device memory, null for 1) and stored, or with */
  uint32_t add;         /* `add` added to what the rows hold */
  const struct AADHipWindowSpan *spans; /* Placed, PlacedStats: each window's crop clipped to and placed by its record (device
                                         * memory, null: every span is (T, 0)) */
  struct AADHipRowStats *stats; /* Stats (w.out may be null), PlacedStats (w.out is null): the level statistics of every row added
                                 * into the table, which the run cleared */
};
/* an object's launch function: defined once, in aad_window_unit.hip.h, and instantiated by the object of <KIND, MODE, HALF> */
template <WindowKind KIND, WindowMode MODE, bool HALF>
void launch_window_object(const WindowUnitRun &r, const WindowLaunch &p, int32_t sample_type, hipStream_t stream);

/* ... and the one way to them: the object of (kind, mode, window_half_type(sample_type)) launches.  sample_type: enum
 * AADHipSampleType, validated by the entry point (window_sample_type_ok, aad_hip_context.hip.h).  Defined in aad_hip_engine.hip */
void launch_window_unit(WindowKind kind, WindowMode mode, const WindowUnitRun &r, const WindowLaunch &p, int32_t sample_type,
                        hipStream_t stream);
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
