/* aad_decode_window_placed.hip - translation unit of the same-format window decoder with a span per window
 * (aad_decode_window_placed.hip.h).  AAD_WINDOW_HALF=0: float32 rows alone (a gain has no int16 rows). */
#include "aad_decode_window_placed.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS, int ST>
static void launch_bits(const WindowPlacedArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.g.w.channels == 1)
    AAD_LAUNCH((decode_window_placed_kernel<BITS, 1, false, ST>), grid, block, lds, stream, a);
  else if (a.g.w.channels == 2 && a.g.w.mid_side)
    AAD_LAUNCH((decode_window_placed_kernel<BITS, 2, true, ST>), grid, block, lds, stream, a);
  else if (a.g.w.channels == 2)
    AAD_LAUNCH((decode_window_placed_kernel<BITS, 2, false, ST>), grid, block, lds, stream, a);
  else
    AAD_LAUNCH((decode_window_placed_kernel<BITS, 0, false, ST>), grid, block, lds, stream, a);
}

template <int ST>
static void launch_type(const WindowPlacedArgs &a, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if (a.g.w.bits == 4) launch_bits<4, ST>(a, grid, block, lds, stream);
  else if (a.g.w.bits == 3) launch_bits<3, ST>(a, grid, block, lds, stream);
  else launch_bits<2, ST>(a, grid, block, lds, stream);
}

template <>
void launch_decode_window_placed_unit<AAD_WINDOW_HALF != 0>(
    const WindowArgs &args, const struct AADHipWindowSpan *spans, const float *gain, uint32_t add, const WindowLaunch &p,
    int32_t sample_type, hipStream_t stream)
{
  const WindowPlacedArgs a = {{args, gain, add, 0}, reinterpret_cast<const uint64_t *>(spans)};
  const dim3 grid(p.grid), block(p.workgroup);
#if AAD_WINDOW_HALF
  if (sample_type == AAD_HIP_SAMPLE_BFLOAT16) launch_type<AAD_HIP_SAMPLE_BFLOAT16>(a, grid, block, p.lds, stream);
  else launch_type<AAD_HIP_SAMPLE_FLOAT16>(a, grid, block, p.lds, stream);
#else
  (void)sample_type;
  launch_type<AAD_HIP_SAMPLE_FLOAT32>(a, grid, block, p.lds, stream);
#endif
}

} /* namespace aad */
