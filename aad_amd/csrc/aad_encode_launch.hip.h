/* aad_encode_launch.hip.h - what one encode run is (EncodeRun) and the way from it and its launch plan (aad_launch_policy.h) to
 * an instantiation of encode_streams_kernel: launch_encode_run<IN, REC>, one instantiation per input layout IN and output REC
 * (aad_encode.hip.h).  aad_hip_engine.hip instantiates the interleaved kernels, aad_encode_units.hip every other pair:
 * the planar ones, the planar reconstruct ones (REC) and those with statistics, one object per pair. */
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

/* One encode run: the kernel arguments, what their table is, where the samples lie and what is written besides the images. */
struct EncodeRun {
  EncodeArgs args;
  bool chain_table = false;      /* args.chains holds a chain table and args.num_streams counts chains (aad_segments.h) */
  PcmLayout in = kInInterleaved; /* interleaved int16 frames, or one row per channel of int16 / float32 samples ... */
  uint64_t channel_stride = 0;   /* ... channel_stride elements apart */
  RecOutput rec = kRecNone;      /* the decoded rows of a planar reconstruct run: none, int16 or float32 ... */
  RecRows rows = {nullptr, nullptr, 0}; /* ... and where they go */
  /* rec with statistics (rec_has_stats, AADHip_PlanarReconstructPlanRunStats): the table, and per chain of a chain table its stream */
  AADHipRowStats *stats = nullptr;
  const uint32_t *stats_stream = nullptr;
};

/* the layout that reads rows of a sample type (enum AADHipSampleType): mono int16 rows ARE interleaved frames, see above */
inline PcmLayout planar_layout(int32_t sample_type, uint32_t channels)
{
  if (sample_type == AAD_HIP_SAMPLE_FLOAT32) return kInPlanarF32;
  return channels == 1 ? kInInterleaved : kInPlanarI16;
}
inline RecOutput rec_output(int32_t sample_type) { return sample_type == AAD_HIP_SAMPLE_FLOAT32 ? kRecF32 : kRecI16; }
/* the same rows with the statistics table (rows == false: the table alone) */
inline RecOutput rec_with_stats(RecOutput rec, bool rows) { return !rows ? kRecStatsOnly : (rec == kRecF32 ? kRecF32Stats : kRecI16Stats); }

/* The kernels of one (IN, REC) by sample width and table kind.  r.in == IN and r.rec == REC: the caller has dispatched on them. */
template <int IN, int REC>
void launch_encode_run(const EncodeRun &r, const EncodeLaunch &p, hipStream_t stream)
{
  KernelArgsFor<IN, REC> a;
  static_cast<EncodeArgs &>(a) = r.args;
  if constexpr (IN != kInInterleaved || REC != kRecNone) a.channel_stride = r.channel_stride;
  if constexpr (REC != kRecNone) {
    a.out = r.rows.out;
    a.out_base = r.rows.base;
    a.out_channel_stride = r.rows.channel_stride;
  }
  if constexpr (rec_has_stats(REC)) {
    a.stats = r.stats;
    a.stats_stream = r.stats_stream;
  }
  auto by_bits = [&](auto seg) {
    constexpr bool SEG = decltype(seg)::value;
    switch (a.bits) {
      case 4: launch_encode<4, SEG, IN, REC>(a, p, stream); break;
      case 3: launch_encode<3, SEG, IN, REC>(a, p, stream); break;
      default: launch_encode<2, SEG, IN, REC>(a, p, stream); break;
    }
  };
  if (r.chain_table) by_bits(std::true_type{});
  else by_bits(std::false_type{});
}

/* Every pair but the interleaved encoders is instantiated by an object of its own (aad_encode_units.hip, compiled once per input
 * sample type and REC, see the Makefile), so that the kernels build side by side.  With a REC the int16-input objects hold
 * IN = kInInterleaved as well. */
extern template void launch_encode_run<kInPlanarI16, kRecNone>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
extern template void launch_encode_run<kInPlanarF32, kRecNone>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
#define AAD_EXTERN_REC_RUN(REC)                                                                                    \
  extern template void launch_encode_run<kInInterleaved, REC>(const EncodeRun &, const EncodeLaunch &, hipStream_t); \
  extern template void launch_encode_run<kInPlanarI16, REC>(const EncodeRun &, const EncodeLaunch &, hipStream_t);   \
  extern template void launch_encode_run<kInPlanarF32, REC>(const EncodeRun &, const EncodeLaunch &, hipStream_t);
AAD_EXTERN_REC_RUN(kRecI16)
AAD_EXTERN_REC_RUN(kRecF32)
AAD_EXTERN_REC_RUN(kRecI16Stats)
AAD_EXTERN_REC_RUN(kRecF32Stats)
AAD_EXTERN_REC_RUN(kRecStatsOnly)
#undef AAD_EXTERN_REC_RUN

} /* namespace aad */

#endif /* AAD_ENCODE_LAUNCH_HIP_H */
