/* aad_convolve.hip.h - the device side of the convolve stage (AADHip_ConvolverResolve, AADHip_ConvolverRun, ...RunGain,
 * ...RunStats; include/aad_hip.h "reverberation"): the resolve kernel in front of a window decode and the FIR kernels behind it.
 * The arithmetic is aad_convolve.h's. */
#ifndef AAD_CONVOLVE_HIP_H
#define AAD_CONVOLVE_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aad_convolve.h"

namespace aad {
namespace convolve {

struct ResolveArgs {
  const uint64_t *windows;  /* struct AADHipWindow[num_windows], device memory */
  const uint64_t *response; /* int64[num_windows], device memory; null: every response is 0 */
  const uint32_t *lead;     /* K - 1 - delay per response, device memory */
  uint64_t num_windows;
  uint32_t num_responses;
  uint64_t *source_windows; /* struct AADHipWindow[num_windows] */
  ConvolveLane *lanes;      /* [num_windows] */
};

/* one response as the FIR kernel sees it */
struct ResponseDesc {
  uint32_t K, q, delay, steps; /* steps: convolve_steps(K) */
  uint64_t offset;             /* first byte of the response's planes (convolve_build_planes), a multiple of 16 */
  int64_t bias;                /* convolve_bias */
};

struct RowsArgs {
  const int16_t *src;            /* [num_windows, channels, source_frames] */
  const ConvolveLane *lanes;     /* [num_windows] */
  const ResponseDesc *responses; /* [num_responses], device memory */
  const int8_t *planes;          /* device memory, 16-byte aligned */
  void *out;                     /* [num_windows, channels, frames] of the sample type */
  uint64_t rows;                 /* num_windows * channels */
  uint32_t channels;
  uint32_t num_responses;
  uint32_t frames;        /* T */
  uint32_t source_frames; /* the source rows' length */
  uint32_t tiles;         /* ceil(T / kConvolveTile) */
};

/* AADHip_ConvolverRunGain: the plain run's arguments and the tables of the loader toolbox */
struct GainArgs {
  RowsArgs r;
  const uint64_t *spans; /* struct AADHipWindowSpan[num_windows] in output frames, or null: every span is (T, 0) */
  const float *gain;     /* [num_windows], or null: every gain is 1 */
};

/* AADHip_ConvolverRunStats: the plain run's arguments (r.out null: no rows) and the tables of the statistics run */
struct StatsArgs {
  RowsArgs r;
  const uint64_t *spans;                   /* struct AADHipWindowSpan[num_windows] in output frames, or null: every span is (T, 0) */
  const unsigned long long *source_stats;  /* struct AADHipRowStats[rows] of the source batch: `count` is read */
  unsigned long long *stats;               /* struct AADHipRowStats[rows], cleared in front of the launch */
};

void launch_resolve(const ResolveArgs &a, hipStream_t stream);
void launch_rows(const RowsArgs &a, int32_t sample_type, hipStream_t stream);
/* sample_type: one of the three float types; add: AAD_HIP_WINDOW_GAIN_ADD */
void launch_rows_gain(const GainArgs &a, int32_t sample_type, bool add, hipStream_t stream);

} /* namespace convolve */

/* the kernels of the statistics run (aad_convolve_stats.hip), in a namespace of their own: aad::convolve holds the kernels of
 * aad_convolve.hip and no other */
namespace convolve_levels {
/* sample_type: any of the four; a.r.out null: statistics only */
void launch_rows_stats(const convolve::StatsArgs &a, int32_t sample_type, hipStream_t stream);
} /* namespace convolve_levels */
} /* namespace aad */

#endif /* AAD_CONVOLVE_HIP_H */
