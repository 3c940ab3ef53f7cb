/* aad_decode_tiled.hip - translation unit of the sector-tiled dense decoder (aad_decode_tiled.hip.h). */
#include "aad_decode_tiled.hip.h"
#include "aad_launch.h"

namespace aad {

template <int BITS>
static void launch_bits(const DecodeArgs &a, dim3 grid, dim3 block, hipStream_t stream)
{
  if (a.channels == 1)
    AAD_LAUNCH((decode_tiled_kernel<BITS, 1, false>), grid, block, 0, stream, a);
  else if (a.mid_side)
    AAD_LAUNCH((decode_tiled_kernel<BITS, 2, true>), grid, block, 0, stream, a);
  else
    AAD_LAUNCH((decode_tiled_kernel<BITS, 2, false>), grid, block, 0, stream, a);
}

void launch_decode_tiled(const DecodeArgs &a, const DecodeLaunch &p, hipStream_t stream)
{
  const dim3 grid(p.grid), block(p.workgroup);
  if (a.bits == 4) launch_bits<4>(a, grid, block, stream);
  else if (a.bits == 3) launch_bits<3>(a, grid, block, stream);
  else launch_bits<2>(a, grid, block, stream);
}

} /* namespace aad */
