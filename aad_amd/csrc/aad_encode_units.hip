/* aad_encode_units.hip - translation unit of every encoder but the interleaved ones (those: aad_hip_engine.hip):
 * encode_streams_kernel (aad_encode.hip.h) over planar int16 / float32 rows, dispatched like the interleaved kernels
 * (launch_encode_run<IN, REC>, aad_encode_launch.hip.h).  The Makefile compiles this file once per pair, so that the kernels build
 * side by side:
 *   AAD_ENCODE_IN_F32  the rows read: 0 - int16 (kInPlanarI16), 1 - float32 (kInPlanarF32)
 *   AAD_ENCODE_REC     what is written besides the images, a RecOutput by value: 0 - nothing (the planar-input encoders,
 *                      AADHip_PlanarEncodePlanRun); 1, 2 - the decoded int16 / float32 rows (planar reconstruct,
 *                      AADHip_PlanarReconstructPlanRun, RecRow); 3, 4 - those rows and the error statistics table, 5 - the table
 *                      alone (AADHip_PlanarReconstructPlanRunStats, RecRowStats)
 * Mono int16 rows are interleaved frames (planar_layout): with a REC the int16-input objects also hold IN = kInInterleaved. */
#include "aad_encode_launch.hip.h"

#if !defined(AAD_ENCODE_IN_F32) || !defined(AAD_ENCODE_REC)
#error "compile with -DAAD_ENCODE_IN_F32=0|1 (int16 or float32 input rows) -DAAD_ENCODE_REC=0..5 (RecOutput: none, int16 rows, float32 rows, those with statistics, statistics alone)"
#endif

namespace aad {
static_assert(AAD_ENCODE_REC >= kRecNone && AAD_ENCODE_REC <= kRecStatsOnly, "AAD_ENCODE_REC: a RecOutput");
#if !AAD_ENCODE_IN_F32 && AAD_ENCODE_REC != 0
template void launch_encode_run<kInInterleaved, AAD_ENCODE_REC>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
#endif
template void launch_encode_run<AAD_ENCODE_IN_F32 ? kInPlanarF32 : kInPlanarI16, AAD_ENCODE_REC>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
}
