/* aad_resample.hip.h - the device side of the resample stage (AADHip_ResamplerResolve, AADHip_ResamplerRun, ...RunGain,
 * ...RunStats; include/aad_hip.h "resample"): the resolve kernel in front of a window decode and the FIR kernels behind it.  The
 * arithmetic is aad_resample.h's. */
#ifndef AAD_RESAMPLE_HIP_H
#define AAD_RESAMPLE_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aad_resample.h"

namespace aad {

struct ResampleResolveArgs {
  const uint64_t *windows; /* struct AADHipWindow[num_windows], device memory */
  const uint64_t *variant; /* int64[num_windows], device memory; null: every variant is 0 */
  const uint16_t *select;  /* [num_streams][variants], device memory */
  const uint16_t *lead;    /* K/2 - 1 per bank, device memory */
  uint64_t num_windows;
  uint64_t num_streams;
  uint32_t variants;
  uint64_t *source_windows; /* struct AADHipWindow[num_windows] */
  ResampleLane *lanes;      /* [num_windows] */
};

/* one bank as the FIR kernel sees it */
struct ResampleBankDesc {
  uint32_t L, M, K;
  uint32_t offset; /* first coefficient, in elements of the coefficient array: phase p's K taps at offset + p * K - of a gathered
                      bank (a wide resampler's, not resample_bank_resident) at offset + p * resample_gather_pitch(K), offset a
                      multiple of 8 */
};

struct ResampleRowsArgs {
  const int16_t *src;            /* [num_windows, channels, source_frames] */
  const ResampleLane *lanes;     /* [num_windows] */
  const ResampleBankDesc *banks; /* [num_banks], device memory */
  const int16_t *coefficients;   /* device memory */
  void *out;                     /* [num_windows, channels, frames] of the sample type */
  uint64_t rows;                 /* num_windows * channels */
  uint32_t channels;
  uint32_t num_banks;
  uint32_t frames;        /* T */
  uint32_t source_frames; /* the source rows' length */
  uint32_t tiles;         /* ceil(T / kResampleTile) */
  uint32_t bank_elements; /* int16 elements of LDS in front of the span: the largest L * resample_lds_stride(K) - of a wide
                             resampler: over its resident banks, and R * resample_lds_stride(K) over the gathered ones */
  uint32_t span_elements; /* the largest resample_span_elements */
};

/* AADHip_ResamplerRunGain / AADHip_ResamplerRunStats: the plain run's arguments and the tables of the loader toolbox */
struct ResampleMixArgs {
  ResampleRowsArgs r;                      /* Stats: r.out may be null */
  const uint64_t *spans;                   /* struct AADHipWindowSpan[num_windows] in OUTPUT frames, or null: every span is (T, 0) */
  const float *gain;                       /* Gain: [num_windows], or null: every gain is 1 */
  const unsigned long long *source_stats;  /* Stats: struct AADHipRowStats[rows] of the source batch */
  unsigned long long *stats;               /* Stats: struct AADHipRowStats[rows], cleared in front of the launch */
  uint32_t scratch_words;                  /* Stats: 32-bit words of LDS in front of the reduction scratch */
  uint32_t round;                          /* the kernels of a wide resampler: R of the gather path, its phase index R words
                                              behind bank and span */
};

/* bytes of the statistics kernel's reduction scratch, behind bank and span on a 16-byte boundary: three 64-bit values a wave */
constexpr uint32_t kResampleStatsScratchBytes = (kResampleThreads / 64) * 3 * 8;
inline uint32_t resample_stats_scratch_offset(uint32_t lds_bytes) { return (lds_bytes + 15u) & ~15u; }

void launch_resample_resolve(const ResampleResolveArgs &a, hipStream_t stream);
/* lds_bytes: 2 * (bank_elements + span_elements); false when the device refuses that much LDS for a workgroup */
bool launch_resample_rows(const ResampleRowsArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream);
/* sample_type: one of the three float types; add: AAD_HIP_WINDOW_GAIN_ADD */
bool launch_resample_rows_gain(const ResampleMixArgs &a, int32_t sample_type, bool add, uint32_t lds_bytes, hipStream_t stream);
/* a.r.out == null: statistics only; lds_bytes as above - the launch adds the scratch and sets a.scratch_words */
bool launch_resample_rows_stats(const ResampleMixArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream);

/* The kernels of a wide resampler (aad_resample_wide.hip), all three over ResampleMixArgs with `round` set; lds_bytes:
 * 2 * (bank_elements + span_elements) + 4 * round */
bool launch_resample_rows_wide(const ResampleMixArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream);
bool launch_resample_rows_gain_wide(const ResampleMixArgs &a, int32_t sample_type, bool add, uint32_t lds_bytes, hipStream_t stream);
bool launch_resample_rows_stats_wide(const ResampleMixArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream);

} /* namespace aad */

#endif /* AAD_RESAMPLE_HIP_H */
