/* aad_encode_stats.hip - translation unit of the planar reconstruct encoders with error statistics
 * (AADHip_PlanarReconstructPlanRunStats): encode_streams_kernel with REC = kRecI16Stats / kRecF32Stats / kRecStatsOnly
 * (aad_encode.hip.h RecRowStats), dispatched like the plain reconstruct encoders (aad_encode_reconstruct.hip).  AAD_REC_IN_F32 picks
 * the input sample type and AAD_STATS_OUT what is written besides the table - 0: int16 rows, 1: float32 rows, 2: nothing: the
 * Makefile compiles this file once per pair, so that the kernels build side by side with the others. */
#include "aad_encode_launch.hip.h"

#if !defined(AAD_REC_IN_F32) || !defined(AAD_STATS_OUT)
#error "compile with -DAAD_REC_IN_F32=0|1 (int16 or float32 input rows) -DAAD_STATS_OUT=0|1|2 (int16 rows, float32 rows, no rows)"
#endif

namespace aad {
constexpr int kRecOfUnit = AAD_STATS_OUT == 2 ? kRecStatsOnly : (AAD_STATS_OUT == 1 ? kRecF32Stats : kRecI16Stats);
#if AAD_REC_IN_F32
template void launch_encode_run<kInPlanarF32, kRecOfUnit>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
#else
template void launch_encode_run<kInInterleaved, kRecOfUnit>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
template void launch_encode_run<kInPlanarI16, kRecOfUnit>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
#endif
}
