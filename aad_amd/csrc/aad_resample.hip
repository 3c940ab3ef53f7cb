/* aad_resample.hip - translation unit of the resample stage's kernels (aad_resample.hip.h) for a plain resampler; a wide one's
 * FIR kernels are aad_resample_wide.hip's.
 *
 * resample_rows_gain_kernel<ST, ADD> and resample_rows_stats_kernel<ST> (AADHip_ResamplerRunGain, AADHip_ResamplerRunStats) are
 *   resample_rows_kernel with another row writer - a gain per window, stored or added, inside a span - and with the rows' exact
 *   level statistics; the tile body (resample_tile) is the one all three share.  The bodies and the notes in front of each are in
 *   aad_resample_tile.hip.h; the kernels here run them over ResampleResident, the bank whole in LDS.
 *
 * resample_resolve_kernel  one thread per window, in front of the window decode: resample_resolve (aad_resample.h) gives the source
 *   window - the window moved K/2 - 1 frames to the front, or to frame 0 - and the lane record {bank, shift} the FIR kernel reads.
 *
 * resample_rows_kernel<ST>  behind the window decode, which has written the int16 source batch: resample_rows_body over
 *   resample_tile (aad_resample_tile.hip.h). */
#include "aad_resample_tile.hip.h"

namespace aad {

__global__ void __launch_bounds__(256) resample_resolve_kernel(ResampleResolveArgs a)
{
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.num_windows) return;
  const ResampleResolved r = resample_resolve(a.windows[2 * w], a.windows[2 * w + 1], a.variant != nullptr ? a.variant[w] : 0,
                                              a.num_streams, a.variants, a.select, a.lead);
  a.source_windows[2 * w] = r.stream;
  a.source_windows[2 * w + 1] = r.src_first;
  a.lanes[w] = r.lane;
}

void launch_resample_resolve(const ResampleResolveArgs &a, hipStream_t stream)
{
  AAD_LAUNCH(resample_resolve_kernel, dim3((uint32_t)((a.num_windows + 255) / 256)), dim3(256), 0, stream, a);
}

template <int ST>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_kernel(ResampleRowsArgs a)
{
  resample_rows_body<ST>(a, ResampleResident{});
}

template <int ST>
static bool launch_type(const ResampleRowsArgs &a, uint32_t lds_bytes, hipStream_t stream)
{
  if (lds_bytes > 65536u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(&resample_rows_kernel<ST>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_bytes) != hipSuccess)
    return false;
  AAD_LAUNCH((resample_rows_kernel<ST>), dim3(resample_grid(a)), dim3(kResampleThreads), lds_bytes, stream, a);
  return true;
}

bool launch_resample_rows(const ResampleRowsArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream)
{
  switch (sample_type) {
    case AAD_HIP_SAMPLE_INT16: return launch_type<AAD_HIP_SAMPLE_INT16>(a, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT32: return launch_type<AAD_HIP_SAMPLE_FLOAT32>(a, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT16: return launch_type<AAD_HIP_SAMPLE_FLOAT16>(a, lds_bytes, stream);
    default: return launch_type<AAD_HIP_SAMPLE_BFLOAT16>(a, lds_bytes, stream);
  }
}

/* ---- rows with gain and spans (AADHip_ResamplerRunGain) ------------------------------------------------------------------------- */

template <int ST, bool ADD>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_gain_kernel(ResampleMixArgs m)
{
  resample_rows_gain_body<ST, ADD>(m, ResampleResident{});
}

template <int ST, bool ADD>
static bool launch_gain_type(const ResampleMixArgs &a, uint32_t lds_bytes, hipStream_t stream)
{
  if (lds_bytes > 65536u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(&resample_rows_gain_kernel<ST, ADD>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return false;
  AAD_LAUNCH((resample_rows_gain_kernel<ST, ADD>), dim3(resample_grid(a.r)), dim3(kResampleThreads), lds_bytes, stream, a);
  return true;
}

bool launch_resample_rows_gain(const ResampleMixArgs &a, int32_t sample_type, bool add, uint32_t lds_bytes, hipStream_t stream)
{
  switch (sample_type) {
    case AAD_HIP_SAMPLE_FLOAT32:
      return add ? launch_gain_type<AAD_HIP_SAMPLE_FLOAT32, true>(a, lds_bytes, stream)
                 : launch_gain_type<AAD_HIP_SAMPLE_FLOAT32, false>(a, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT16:
      return add ? launch_gain_type<AAD_HIP_SAMPLE_FLOAT16, true>(a, lds_bytes, stream)
                 : launch_gain_type<AAD_HIP_SAMPLE_FLOAT16, false>(a, lds_bytes, stream);
    default:
      return add ? launch_gain_type<AAD_HIP_SAMPLE_BFLOAT16, true>(a, lds_bytes, stream)
                 : launch_gain_type<AAD_HIP_SAMPLE_BFLOAT16, false>(a, lds_bytes, stream);
  }
}

/* ---- level statistics of the resampled rows (AADHip_ResamplerRunStats) ---------------------------------------------------------- */

template <int ST>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_stats_kernel(ResampleMixArgs m)
{
  resample_rows_stats_body<ST>(m, ResampleResident{});
}

template <int ST>
static bool launch_stats_type(ResampleMixArgs a, uint32_t lds_bytes, hipStream_t stream)
{
  const uint32_t scratch = resample_stats_scratch_offset(lds_bytes);
  a.scratch_words = scratch / 4;
  lds_bytes = scratch + kResampleStatsScratchBytes;
  if (lds_bytes > 65536u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(&resample_rows_stats_kernel<ST>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_bytes) != hipSuccess)
    return false;
  AAD_LAUNCH((resample_rows_stats_kernel<ST>), dim3(resample_grid(a.r)), dim3(kResampleThreads), lds_bytes, stream, a);
  return true;
}

bool launch_resample_rows_stats(const ResampleMixArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream)
{
  if (a.r.out == nullptr) return launch_stats_type<kResampleNoRows>(a, lds_bytes, stream);
  switch (sample_type) {
    case AAD_HIP_SAMPLE_INT16: return launch_stats_type<AAD_HIP_SAMPLE_INT16>(a, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT32: return launch_stats_type<AAD_HIP_SAMPLE_FLOAT32>(a, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT16: return launch_stats_type<AAD_HIP_SAMPLE_FLOAT16>(a, lds_bytes, stream);
    default: return launch_stats_type<AAD_HIP_SAMPLE_BFLOAT16>(a, lds_bytes, stream);
  }
}

} /* namespace aad */
