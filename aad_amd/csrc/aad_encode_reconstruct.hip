/* aad_encode_reconstruct.hip - translation unit of the planar reconstruct encoders (AADHip_PlanarReconstructPlanRun):
 * encode_streams_kernel with REC = kRecI16 / kRecF32 (aad_encode.hip.h RecRow) over planar int16 / float32 rows, dispatched like
 * the planar encoders (launch_encode_run, aad_encode_launch.hip.h).  AAD_REC_IN_F32 and AAD_REC_OUT_F32 pick the pair of sample
 * types this object instantiates: the Makefile compiles this file once per pair.  Mono int16 rows are interleaved frames
 * (planar_layout): the int16-input objects also hold IN = kInInterleaved. */
#include "aad_encode_launch.hip.h"

#if !defined(AAD_REC_IN_F32) || !defined(AAD_REC_OUT_F32)
#error "compile with -DAAD_REC_IN_F32=0|1 -DAAD_REC_OUT_F32=0|1 (int16 or float32 input rows, output rows)"
#endif

namespace aad {
constexpr int kRecOfUnit = AAD_REC_OUT_F32 ? kRecF32 : kRecI16;
#if AAD_REC_IN_F32
template void launch_encode_run<kInPlanarF32, kRecOfUnit>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
#else
template void launch_encode_run<kInInterleaved, kRecOfUnit>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
template void launch_encode_run<kInPlanarI16, kRecOfUnit>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
#endif
}
