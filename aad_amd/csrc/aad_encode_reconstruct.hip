/* aad_encode_reconstruct.hip - translation unit of the planar reconstruct encoders (AADHip_PlanarReconstructPlanRun):
 * encode_streams_kernel with REC = kRecI16 / kRecF32 (aad_encode.hip.h RecRow) over planar int16 / float32 rows, dispatched like
 * the planar encoders (aad_encode_launch.hip.h).  AAD_REC_IN_F32 and AAD_REC_OUT_F32 pick the two sample types: the Makefile
 * compiles this file once per pair.  Mono int16 rows are interleaved frames: those plans run IN = kInInterleaved. */
#include "aad_encode_launch.hip.h"

#if !defined(AAD_REC_IN_F32) || !defined(AAD_REC_OUT_F32)
#error "compile with -DAAD_REC_IN_F32=0|1 -DAAD_REC_OUT_F32=0|1 (int16 or float32 input rows, output rows)"
#endif

namespace aad {

namespace {
template <int IN, int REC>
void launch_rec(const RecEncodeArgs &a, const EncodeLaunch &p, bool segmented, hipStream_t stream)
{
  if (segmented) {
    switch (a.bits) {
      case 4: launch_encode<4, true, IN, REC>(a, p, stream); break;
      case 3: launch_encode<3, true, IN, REC>(a, p, stream); break;
      default: launch_encode<2, true, IN, REC>(a, p, stream); break;
    }
  } else {
    switch (a.bits) {
      case 4: launch_encode<4, false, IN, REC>(a, p, stream); break;
      case 3: launch_encode<3, false, IN, REC>(a, p, stream); break;
      default: launch_encode<2, false, IN, REC>(a, p, stream); break;
    }
  }
}
} /* namespace */

#if AAD_REC_IN_F32 && AAD_REC_OUT_F32
void launch_reconstruct_f32_f32(const EncodeArgs &args, uint64_t channel_stride, const RecRows &out, const EncodeLaunch &p, bool segmented, hipStream_t stream)
#elif AAD_REC_IN_F32
void launch_reconstruct_f32_i16(const EncodeArgs &args, uint64_t channel_stride, const RecRows &out, const EncodeLaunch &p, bool segmented, hipStream_t stream)
#elif AAD_REC_OUT_F32
void launch_reconstruct_i16_f32(const EncodeArgs &args, uint64_t channel_stride, const RecRows &out, const EncodeLaunch &p, bool segmented, hipStream_t stream)
#else
void launch_reconstruct_i16_i16(const EncodeArgs &args, uint64_t channel_stride, const RecRows &out, const EncodeLaunch &p, bool segmented, hipStream_t stream)
#endif
{
  constexpr int REC = AAD_REC_OUT_F32 ? kRecF32 : kRecI16;
  RecEncodeArgs a;
  static_cast<EncodeArgs &>(a) = args;
  a.channel_stride = channel_stride;
  a.out = out.out;
  a.out_base = out.base;
  a.out_channel_stride = out.channel_stride;
#if AAD_REC_IN_F32
  launch_rec<kInPlanarF32, REC>(a, p, segmented, stream);
#else
  if (a.channels == 1) launch_rec<kInInterleaved, REC>(a, p, segmented, stream);
  else launch_rec<kInPlanarI16, REC>(a, p, segmented, stream);
#endif
}

} /* namespace aad */
