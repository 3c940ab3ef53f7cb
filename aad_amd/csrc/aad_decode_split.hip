/*
 * aad_decode_split.hip - translation unit of the split (two-strand) quad decoder.
 *
 * Separate from aad_hip_engine.hip only because of one compiler flag: with LLVM's
 * "iterative-ilp" machine-scheduling strategy the prediction recurrence's chunk body comes out
 * 7 % faster on gfx950 (0.0452 -> 0.0420 ms for the bench batch, same box, bit-identical output;
 * the strategy alternates the two independent strands of a sample instead of emitting them one
 * after the other, and a lone wave pays an extra cycle for every instruction that reads the
 * result of the one just before it).  The same flag makes no difference to the encoder and is
 * not applied to the other kernels.
 */
#include <cstring>

#include "aad_decode_split.hip.h"
#include "aad_launch.h"

namespace aad {

/* the most dynamic LDS a ROLE instantiation is launched with: sixteen rows for kLdsResidualMax coded samples */
constexpr uint32_t kRoleLdsMax = 16u * (kLdsResidualMax + 4u) * (uint32_t)sizeof(int32_t);

/* a ROLE kernel's rows pass the 64 KB a kernel may have of dynamic LDS without asking: its limit is raised once per kernel */
template <int BITS, int CHF, bool MS, bool LDSRES>
static void launch_role(const SplitDecodeArgs &sa, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream)
{
  if constexpr (LDSRES) {
    static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void *>(&decode_split_kernel<BITS, CHF, MS, true, true>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRoleLdsMax);
    (void)raised; /* had it failed, the launch of rows beyond 64 KB fails and the run reports it */
  }
  AAD_LAUNCH((decode_split_kernel<BITS, CHF, MS, LDSRES, true>), grid, block, lds, stream, sa);
}

template <int BITS, bool LDSRES>
static void launch_bits(const SplitDecodeArgs &sa, dim3 grid, dim3 block, uint32_t role_lds, bool role, hipStream_t stream)
{
  if (role) {
    if (sa.d.channels == 1) launch_role<BITS, 1, false, LDSRES>(sa, grid, block, role_lds, stream);
    else if (sa.d.mid_side) launch_role<BITS, 2, true, LDSRES>(sa, grid, block, role_lds, stream);
    else launch_role<BITS, 2, false, LDSRES>(sa, grid, block, role_lds, stream);
    return;
  }
  if (sa.d.channels == 1)
    AAD_LAUNCH((decode_split_kernel<BITS, 1, false, LDSRES>), grid, block, 0, stream, sa);
  else if (sa.d.mid_side)
    AAD_LAUNCH((decode_split_kernel<BITS, 2, true, LDSRES>), grid, block, 0, stream, sa);
  else
    AAD_LAUNCH((decode_split_kernel<BITS, 2, false, LDSRES>), grid, block, 0, stream, sa);
}

void launch_decode_split(const DecodeArgs &args, const DecodeLaunch &p, int32_t *residual, hipStream_t stream)
{
  SplitDecodeArgs sa;
  sa.d = args;
  sa.residual = residual;
  sa.residual_stride = p.residual_stride;
  const bool role = p.simd_role != 0;
  sa.simd = role ? (uint8_t)(p.simd_role - 1u) : 0;
  sa.reserved = 0;
  sa.lds_row = (uint16_t)p.lds_row; /* at most kLdsResidualMax + 4 */
  const dim3 grid(p.grid), block(p.workgroup);
  const bool lds = p.kernel == DecodeKernel::SplitLds;
  switch (args.bits) {
    case 4: lds ? launch_bits<4, true>(sa, grid, block, p.lds, role, stream) : launch_bits<4, false>(sa, grid, block, 0, role, stream); break;
    case 3: lds ? launch_bits<3, true>(sa, grid, block, p.lds, role, stream) : launch_bits<3, false>(sa, grid, block, 0, role, stream); break;
    default: lds ? launch_bits<2, true>(sa, grid, block, p.lds, role, stream) : launch_bits<2, false>(sa, grid, block, 0, role, stream); break;
  }
}

} /* namespace aad */

#if AAD_PHASE_TIMING
/* measurement builds only: copy out and reset the phase log of this unit's kernels
 * (kernel entry | tables written | barrier | strand 1 done | barrier | header parsed, first frames out |
 *  first loads + prime | chunk loop | tail) */
extern "C" uint32_t AADHipDebug_ReadSplitPhaseTimes(uint64_t *out, uint32_t capacity)
{
  uint32_t n = 0, zero = 0;
  uint64_t host[512];
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(aad::g_phase_count), sizeof(n));
  (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(aad::g_phase_times), sizeof(host));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(aad::g_phase_count), &zero, sizeof(zero));
  if (n > capacity) n = capacity;
  memcpy(out, host, sizeof(uint64_t) * n);
  return n;
}
#endif
