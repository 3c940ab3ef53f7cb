/* aad_spectrogram.hip - translation unit of the spectrogram stage's kernel over rows as they lie (AADHip_SpectrogramRun), in
 * namespace aad::spectrum: spectrum_rows_kernel<MEL>, MEL false for the power spectrum and true for the filterbank behind it.  The
 * kernel's body is aad_spectrogram_rows.hip.h's rows_body with the plain stager; the unit compiles with -ffp-contract=off. */
#include "aad_spectrogram_rows.hip.h"

namespace aad {
namespace spectrum {

template <bool MEL>
__global__ void __launch_bounds__(kSpectrumThreads) spectrum_rows_kernel(Args a)
{
  rows_body<MEL>(a, PlainStager{a});
}

bool launch(const Args &a, hipStream_t stream)
{
  return a.num_filters != 0 ? launch_rows(&spectrum_rows_kernel<true>, a, a, true, stream)
                            : launch_rows(&spectrum_rows_kernel<false>, a, a, false, stream);
}

} /* namespace spectrum */
} /* namespace aad */
