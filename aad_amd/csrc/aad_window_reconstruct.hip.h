/* aad_window_reconstruct.hip.h - the device side of a window reconstruct run (AADHip_WindowReconstructPlanRun) in front of the
 * encoders: the resolve kernel, which writes the lane tables of the encoder launch from the window table and zeroes the row
 * tails.  The encoders themselves are the planar reconstruct kernels, unchanged (aad_encode_launch.hip.h). */
#ifndef AAD_WINDOW_RECONSTRUCT_HIP_H
#define AAD_WINDOW_RECONSTRUCT_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aad_segments.h" /* ChainDesc */
#include "aad_windows.h"

namespace aad {

struct WindowResolveArgs {
  const AADHipStreamDesc *sources; /* the plan's source table: pcm_offset and num_samples are read */
  const uint64_t *windows;         /* struct AADHipWindow[num_windows], device memory */
  uint64_t num_sources;
  uint64_t num_windows;
  WindowGeometry g;
  /* resolve: one entry per lane (num_windows * g.chains_per_window) */
  void *table;            /* AADHipStreamDesc (g.segment_blocks == 0) or ChainDesc */
  uint64_t *out_base;
  uint32_t *stats_stream;
  /* tails: the rows, `channels` of g.frames elements per window; null: the run writes no rows */
  void *out;
  uint64_t out_channel_stride;
  uint32_t channels;
  uint32_t out_float32;
};

/* through AAD_LAUNCH: the run's first launch carries its start event (aad_launch.h) */
void launch_window_resolve(const WindowResolveArgs &a, hipStream_t stream);

} /* namespace aad */

#endif /* AAD_WINDOW_RECONSTRUCT_HIP_H */
