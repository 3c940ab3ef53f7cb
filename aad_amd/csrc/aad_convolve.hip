/* aad_convolve.hip - translation unit of the convolve stage's kernels (aad_convolve.hip.h), in namespace aad::convolve.
 *
 * convolve_resolve_kernel  one thread per window, in front of the window decode: convolve_resolve (aad_convolve.h) gives the source
 *   window - the window moved K - 1 - delay frames to the front, or to frame 0 - and the lane record {response, shift} the FIR
 *   kernel reads.
 *
 * convolve_rows_kernel<ST>  behind the window decode, which has written the int16 source batch: rows_body over convolve_tile
 *   (aad_convolve_tile.hip.h), the exact sums as int8 matrix products.
 *
 * convolve_rows_gain_kernel<ST, ADD> (AADHip_ConvolverRunGain) is convolve_rows_kernel with the row writer of the resample stage's
 *   gain kernel - a gain per window, stored or added, inside a span. */
#include "aad_convolve_tile.hip.h"

namespace aad {
namespace convolve {

__global__ void __launch_bounds__(256) convolve_resolve_kernel(ResolveArgs a)
{
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.num_windows) return;
  const ConvolveResolved r =
      convolve_resolve(a.windows[2 * w], a.windows[2 * w + 1], a.response != nullptr ? a.response[w] : 0, a.num_responses, a.lead);
  a.source_windows[2 * w] = r.stream;
  a.source_windows[2 * w + 1] = r.src_first;
  a.lanes[w] = r.lane;
}

void launch_resolve(const ResolveArgs &a, hipStream_t stream)
{
  AAD_LAUNCH(convolve_resolve_kernel, dim3((uint32_t)((a.num_windows + 255) / 256)), dim3(256), 0, stream, a);
}

template <int ST>
__global__ void __launch_bounds__(kConvolveThreads) convolve_rows_kernel(RowsArgs a)
{
  rows_body<ST>(a);
}

template <int ST>
static void launch_type(const RowsArgs &a, hipStream_t stream)
{
  AAD_LAUNCH((convolve_rows_kernel<ST>), dim3(grid(a)), dim3(kConvolveThreads), 0, stream, a);
}

void launch_rows(const RowsArgs &a, int32_t sample_type, hipStream_t stream)
{
  switch (sample_type) {
    case AAD_HIP_SAMPLE_INT16: return launch_type<AAD_HIP_SAMPLE_INT16>(a, stream);
    case AAD_HIP_SAMPLE_FLOAT32: return launch_type<AAD_HIP_SAMPLE_FLOAT32>(a, stream);
    case AAD_HIP_SAMPLE_FLOAT16: return launch_type<AAD_HIP_SAMPLE_FLOAT16>(a, stream);
    default: return launch_type<AAD_HIP_SAMPLE_BFLOAT16>(a, stream);
  }
}

template <int ST, bool ADD>
__global__ void __launch_bounds__(kConvolveThreads) convolve_rows_gain_kernel(GainArgs m)
{
  rows_gain_body<ST, ADD>(m);
}

template <int ST, bool ADD>
static void launch_gain_type(const GainArgs &a, hipStream_t stream)
{
  AAD_LAUNCH((convolve_rows_gain_kernel<ST, ADD>), dim3(grid(a.r)), dim3(kConvolveThreads), 0, stream, a);
}

void launch_rows_gain(const GainArgs &a, int32_t sample_type, bool add, hipStream_t stream)
{
  switch (sample_type) {
    case AAD_HIP_SAMPLE_FLOAT32:
      return add ? launch_gain_type<AAD_HIP_SAMPLE_FLOAT32, true>(a, stream) : launch_gain_type<AAD_HIP_SAMPLE_FLOAT32, false>(a, stream);
    case AAD_HIP_SAMPLE_FLOAT16:
      return add ? launch_gain_type<AAD_HIP_SAMPLE_FLOAT16, true>(a, stream) : launch_gain_type<AAD_HIP_SAMPLE_FLOAT16, false>(a, stream);
    default:
      return add ? launch_gain_type<AAD_HIP_SAMPLE_BFLOAT16, true>(a, stream)
                 : launch_gain_type<AAD_HIP_SAMPLE_BFLOAT16, false>(a, stream);
  }
}

} /* namespace convolve */
} /* namespace aad */
