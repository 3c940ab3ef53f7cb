/* aad_spectrogram.hip.h - what the host side of the spectrogram stage (aad_fir_stage.hip) hands to its kernels
 * (aad_spectrogram.hip, aad_spectrogram_mix.hip): the arguments and the launches.  No device code - that is
 * aad_spectrogram_rows.hip.h's.  The arithmetic is aad_spectrogram.h's. */
#ifndef AAD_SPECTROGRAM_HIP_H
#define AAD_SPECTROGRAM_HIP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aad_spectrogram.h"

namespace aad {
namespace spectrum {

struct Args {
  const int16_t *rows; /* row r at rows + r * row_pitch, `frames` elements */
  uint64_t row_pitch, num_rows;
  uint32_t frames, num_frames, hop; /* T, F, H */
  uint32_t steps, pairs, bins, q;   /* spectrum_steps(W), spectrum_pairs(n_fft), B, the scale exponent */
  SpectrumGeometry g;
  uint32_t tiles;           /* ceil(F / g.tile_frames) */
  const int8_t *planes;     /* spectrum_build_planes, device memory, 16-byte aligned */
  const long long *consts;  /* spectrum_column_constants */
  uint32_t num_filters;     /* M; 0: `out` is P itself, [num_rows, F, B] */
  const SpectrumBand *bands;  /* [M] */
  const float *weights;       /* spectrum_pack_weights */
  const uint32_t *tile_first; /* spectrum_tile_lists: [pairs + 1] */
  const uint32_t *tile_list;
  float *out; /* [num_rows, F, M] */
};

/* false: the device refuses the launch's LDS (spectrum_lds_bytes) */
bool launch(const Args &a, hipStream_t stream);

} /* namespace spectrum */

namespace spectrum_mix {

/* AADHip_SpectrogramRunMix (aad_spectrogram_mix.hip): s.rows / s.row_pitch are a's; group G = row / rows_per_gain */
struct Args {
  spectrum::Args s;
  const int16_t *rows_b; /* row r at rows_b + r * row_pitch_b, read below the group's Le alone */
  uint64_t row_pitch_b;
  uint32_t rows_per_gain;
  const float *gain_a, *gain_b; /* [num_rows / rows_per_gain]; null: every gain 1 */
  const uint64_t *spans;        /* AADHipWindowSpan records, (L, o) of group G at spans[2 G]; null: every span (T, 0) */
};

/* false: the device refuses the launch's LDS (spectrum_lds_bytes) */
bool launch(const Args &a, hipStream_t stream);

} /* namespace spectrum_mix */
} /* namespace aad */

#endif /* AAD_SPECTROGRAM_HIP_H */
