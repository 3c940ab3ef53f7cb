/* aad_encode_planar.hip - translation unit of the planar-input encoders (AADHip_PlanarEncodePlanRun): encode_streams_kernel with
 * IN = kInPlanarI16 / kInPlanarF32 (aad_encode.hip.h), dispatched like the interleaved kernels (aad_encode_launch.hip.h).
 * AAD_ENCODE_PLANAR_F32 picks the sample type: the Makefile compiles this file once per type, so the two sets of kernels build
 * side by side. */
#include "aad_encode_launch.hip.h"

#ifndef AAD_ENCODE_PLANAR_F32
#error "compile with -DAAD_ENCODE_PLANAR_F32=0 (int16 rows) or =1 (float32 rows)"
#endif

namespace aad {

#if AAD_ENCODE_PLANAR_F32
void launch_encode_planar_f32(const EncodeArgs &args, uint64_t channel_stride, const EncodeLaunch &p, bool segmented, hipStream_t stream)
#else
void launch_encode_planar_i16(const EncodeArgs &args, uint64_t channel_stride, const EncodeLaunch &p, bool segmented, hipStream_t stream)
#endif
{
  constexpr int IN = AAD_ENCODE_PLANAR_F32 ? kInPlanarF32 : kInPlanarI16;
  PlanarEncodeArgs a;
  static_cast<EncodeArgs &>(a) = args;
  a.channel_stride = channel_stride;
  if (segmented) {
    switch (a.bits) {
      case 4: launch_encode<4, true, IN>(a, p, stream); break;
      case 3: launch_encode<3, true, IN>(a, p, stream); break;
      default: launch_encode<2, true, IN>(a, p, stream); break;
    }
  } else {
    switch (a.bits) {
      case 4: launch_encode<4, false, IN>(a, p, stream); break;
      case 3: launch_encode<3, false, IN>(a, p, stream); break;
      default: launch_encode<2, false, IN>(a, p, stream); break;
    }
  }
}

} /* namespace aad */
