/* aad_spectrogram_mix.hip - translation unit of the spectrogram stage's kernel over a mix of two int16 row batches
 * (AADHip_SpectrogramRunMix, include/aad_hip.h "spectrogram", paragraph "mix"), in namespace aad::spectrum_mix:
 * spectrum_mix_rows_kernel<MEL>, MEL as in aad_spectrogram.hip.  The kernel's body is aad_spectrogram_rows.hip.h's rows_body; what
 * this unit adds is the stager: row r of the run belongs to group G = r / rows_per_gain - of the item loop's 64-bit row - whose
 * gains and span (L, o) are read once per item, NULL tables by uniform branches, and sample j is spectrum_mix_sample
 * (aad_spectrogram.h) of a[j] and, for o <= j < o + Le, of b[j - o].  The span (L, o) is clipped in 64 bits (spectrum_mix_span) to
 * 32-bit (first, length), which every element is compared with, so its edges lie at any element in both staging modes; b is read
 * at its own pitch, two bytes at a time, at indices below Le alone, a at indices below `frames`, as rows_body asks.  The unit
 * compiles with -ffp-contract=off. */
#include "aad_spectrogram_rows.hip.h"

namespace aad {
namespace spectrum_mix {

struct MixStager {
  struct Row {
    const int16_t *a, *b;
    float ga, gb;
    uint32_t first, length; /* b's span: elements first ... first + length - 1 of the row, all below `frames` */
    __device__ __forceinline__ int16_t sample(uint64_t j) const
    {
      const uint32_t i = (uint32_t)j - first; /* j < frames: 32 bits hold it; below `first` the difference wraps past length */
      const bool inside = i < length;
      return spectrum_mix_sample(ga, a[j], gb, inside ? b[i] : (int16_t)0, inside);
    }
  };
  const Args &m;
  __device__ __forceinline__ Row row(uint64_t r) const
  {
    const uint64_t G = r / m.rows_per_gain;
    const uint64_t L = m.spans != nullptr ? m.spans[2 * G] : m.s.frames, o = m.spans != nullptr ? m.spans[2 * G + 1] : 0;
    const uint32_t Le = spectrum_mix_span(L, o, m.s.frames);
    return Row{m.s.rows + r * m.s.row_pitch, m.rows_b + r * m.row_pitch_b, m.gain_a != nullptr ? m.gain_a[G] : 1.0f,
               m.gain_b != nullptr ? m.gain_b[G] : 1.0f, Le != 0 ? (uint32_t)o : 0u, Le};
  }
};

template <bool MEL>
__global__ void __launch_bounds__(kSpectrumThreads) spectrum_mix_rows_kernel(Args m)
{
  spectrum::rows_body<MEL>(m.s, MixStager{m});
}

bool launch(const Args &m, hipStream_t stream)
{
  return m.s.num_filters != 0 ? spectrum::launch_rows(&spectrum_mix_rows_kernel<true>, m, m.s, true, stream)
                              : spectrum::launch_rows(&spectrum_mix_rows_kernel<false>, m, m.s, false, stream);
}

} /* namespace spectrum_mix */
} /* namespace aad */
