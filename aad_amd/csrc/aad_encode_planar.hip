/* aad_encode_planar.hip - translation unit of the planar-input encoders (AADHip_PlanarEncodePlanRun): encode_streams_kernel with
 * IN = kInPlanarI16 / kInPlanarF32 (aad_encode.hip.h), dispatched like the interleaved kernels (launch_encode_run,
 * aad_encode_launch.hip.h).  AAD_ENCODE_PLANAR_F32 picks the sample type this object instantiates: the Makefile compiles this
 * file once per type, so the two sets of kernels build side by side. */
#include "aad_encode_launch.hip.h"

#ifndef AAD_ENCODE_PLANAR_F32
#error "compile with -DAAD_ENCODE_PLANAR_F32=0 (int16 rows) or =1 (float32 rows)"
#endif

namespace aad {
template void launch_encode_run<AAD_ENCODE_PLANAR_F32 ? kInPlanarF32 : kInPlanarI16, kRecNone>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
}
