/* aad_encode_launch.hip.h - from an encode plan (aad_launch_policy.h) to an instantiation of encode_streams_kernel, for one input
 * layout IN (aad_encode.hip.h).  aad_hip_engine.hip instantiates the interleaved kernels, aad_encode_planar.hip the planar ones,
 * aad_encode_reconstruct.hip the planar reconstruct ones (REC). */
#ifndef AAD_ENCODE_LAUNCH_HIP_H
#define AAD_ENCODE_LAUNCH_HIP_H

#include "aad_encode.hip.h"
#include "aad_launch.h"

namespace aad {

/* encode_streams_kernel by channels and M/S; RING: the dense encoders whose output goes through the rows' byte rings
 * (aad_encode.hip.h ByteRing), mono / stereo only; SEG: the chains of a segmented plan.  Planar int16 mono input is the
 * interleaved layout itself: its plans run the interleaved kernels and no planar instantiation exists for it (reconstruct: the
 * interleaved instantiation with REC serves mono int16 alone). */
template <int BITS, bool QUAD, bool TRIALS, bool DUAL, bool RING = false, bool SEG = false, int IN = kInInterleaved, int REC = kRecNone>
void launch_encode_mapped(const KernelArgsFor<IN, REC> &a, const EncodeLaunch &p, hipStream_t stream)
{
  const dim3 grid(p.grid), block(p.workgroup);
  if (a.channels == 1) {
    if constexpr (IN != kInPlanarI16)
      AAD_LAUNCH((encode_streams_kernel<BITS, 1, false, QUAD, TRIALS, DUAL, RING, SEG, IN, REC>), grid, block, p.lds, stream, a);
  } else if constexpr (IN == kInInterleaved && REC != kRecNone) {
  } else if (a.channels == 2 && a.mid_side)
    AAD_LAUNCH((encode_streams_kernel<BITS, 2, true, QUAD, TRIALS, DUAL, RING, SEG, IN, REC>), grid, block, p.lds, stream, a);
  else if (a.channels == 2)
    AAD_LAUNCH((encode_streams_kernel<BITS, 2, false, QUAD, TRIALS, DUAL, RING, SEG, IN, REC>), grid, block, p.lds, stream, a);
  else if constexpr (!QUAD && !RING)
    AAD_LAUNCH((encode_streams_kernel<BITS, 0, false, false, TRIALS, false, false, SEG, IN, REC>), grid, block, p.lds, stream, a);
}

template <int BITS, bool SEG, int IN = kInInterleaved, int REC = kRecNone>
void launch_encode(const KernelArgsFor<IN, REC> &a, const EncodeLaunch &p, hipStream_t stream)
{
  if (p.trials) {
    if (p.kernel == EncodeKernel::QuadDual) {
      if constexpr (REC == kRecNone) launch_encode_mapped<BITS, true, true, true, false, SEG, IN>(a, p, stream); /* REC: never planned */
    } else if (p.kernel == EncodeKernel::Quad) {
      launch_encode_mapped<BITS, true, true, false, false, SEG, IN, REC>(a, p, stream);
    } else {
      launch_encode_mapped<BITS, false, true, false, false, SEG, IN, REC>(a, p, stream);
    }
  } else if (p.kernel == EncodeKernel::Quad) {
    launch_encode_mapped<BITS, true, false, false, false, SEG, IN, REC>(a, p, stream);
  } else if (p.kernel == EncodeKernel::DenseRing) {
    if constexpr (!SEG && REC == kRecNone) launch_encode_mapped<BITS, false, false, false, true, false, IN>(a, p, stream); /* SEG: ring_ok = 0, REC: never planned */
  } else {
    launch_encode_mapped<BITS, false, false, false, false, SEG, IN, REC>(a, p, stream);
  }
}

} /* namespace aad */

#endif /* AAD_ENCODE_LAUNCH_HIP_H */
