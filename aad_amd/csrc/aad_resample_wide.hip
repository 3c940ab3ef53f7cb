/* aad_resample_wide.hip - the FIR kernels of a wide resampler (AADHip_ResamplerCreateWide, include/aad_hip.h "resample"): the
 * bodies of aad_resample_tile.hip.h over a tile that takes one of two paths per (row, tile of 1024 outputs), by the row's bank
 * alone and so the same for the whole workgroup -
 *
 *   resident   the bank passes resample_bank_resident (what AADHip_ResamplerCreate accepts): resample_tile, the plain
 *              resampler's code, the bank whole in LDS;
 *   gathered   any other bank: resample_tile_gathered below.  A tile of 1024 outputs reads at most 1024 of the bank's L phases,
 *              so only those rows come into LDS, a ROUND of R consecutive outputs at a time (R = a.round: 64, 128 or 256, fixed
 *              per resampler on the host by resample_gather_round, aad_resample.h).
 *
 * A round: the threads that own its outputs - output tile + tid + 256 j belongs to round (tid + 256 j) / R of the tile and is
 * row t = (tid + 256 j) mod R of it - publish their phase p in the phase index; after a barrier all 256 threads copy the rows
 * index[t], t < R, of the bank from global memory (L2: a bank is read by every workgroup of its ratio; the device's copy of a
 * gathered bank has its rows resample_gather_pitch(K) apart, on 16-byte boundaries) to t * stride int16 of the bank region,
 * resample_lds_stride as for a whole bank, in 16-byte pieces, adjacent threads adjacent pieces of a row; after a second barrier the owners run resample_dot over row t, the inner loop
 * of the resident path, and emit.  The next round's index writes need no third barrier - the index is read before the second
 * barrier only, the rows are written after the next first.  The span of the source row is staged once per tile, as resident. */
#include "aad_resample_tile.hip.h"

namespace aad {

/* 16-byte pieces a thread copies per turn of a round's copy loop, their index reads and global loads issued together.  With 4-byte
 * loads, 16 a turn - a whole round in two turns - measured no faster than 4: the copy is not bound by the latency of L2 but by the
 * number of load instructions, hence the 16-byte pieces (DESIGN.md "Wide resampler") */
constexpr int kResampleGatherBatch = 4;

template <class Emit>
__device__ __forceinline__ void resample_tile_gathered(const ResampleRowsArgs &a, const ResampleBankDesc &d, uint32_t round,
                                                       uint32_t *row_words, uint32_t *span_words, uint32_t *index, uint64_t row,
                                                       uint32_t shift, uint32_t n0, uint32_t n_end, Emit emit)
{
  const uint32_t tid = threadIdx.x;
  const uint32_t half = d.K / 2, stride_words = resample_lds_stride(d.K) / 2;
  __syncthreads(); /* the previous item's reads are done */
  const ResampleSpanAt at = resample_stage_span(a, d, span_words, row, shift, n0, n_end);
  /* the device copy of a gathered bank has its rows resample_gather_pitch(K) apart, on 16-byte boundaries: a row is `quads` 16-byte
   * pieces.  Thread tid copies pieces tid, tid + 256, ... of the round's rows laid end to end: piece c of row t, stepped without
   * a division */
  const uint32_t quads = resample_gather_pitch(d.K) / 8;
  const uint4 *const g = reinterpret_cast<const uint4 *>(a.coefficients + d.offset);
  const uint32_t t_first = tid / quads, c_first = tid - t_first * quads;
  const uint32_t dt = kResampleThreads / quads, dc = kResampleThreads - dt * quads;
  const uint32_t step = kResampleThreads * d.M, di = step / d.L, dp = step - di * d.L;
  uint32_t n = n0 + tid;
  const uint32_t nm = n * d.M;
  uint32_t i = nm / d.L, p = nm - i * d.L;
#pragma unroll 1
  for (uint32_t j = 0; j < kResamplePerThread && n0 + j * kResampleThreads < n_end; j++, n += kResampleThreads) {
    const ResampleGatherSlot slot = resample_gather_slot(j * kResampleThreads + tid, round);
    const uint32_t t_mine = slot.row;
#pragma unroll 1
    for (uint32_t first = j * kResampleThreads; first < (j + 1) * kResampleThreads; first += round) {
      const uint32_t base = n0 + first; /* the round's first output */
      if (base >= n_end) break;
      const uint32_t rows = n_end - base < round ? n_end - base : round;
      const bool mine = slot.round == resample_gather_slot(first, round).round && t_mine < rows;
      if (mine) index[t_mine] = p;
      __syncthreads(); /* the index is whole; the last round's reads of the rows are done */
      uint32_t t = t_first, c = c_first;
      while (t < rows) { /* kResampleGatherBatch pieces a turn: their index reads and global loads are issued together */
        uint32_t tt[kResampleGatherBatch], cc[kResampleGatherBatch];
        uint4 v[kResampleGatherBatch];
#pragma unroll
        for (int u = 0; u < kResampleGatherBatch; u++) {
          tt[u] = t;
          cc[u] = c;
          t += dt;
          c += dc;
          if (c >= quads) {
            c -= quads;
            t += 1;
          }
        }
#pragma unroll
        for (int u = 0; u < kResampleGatherBatch; u++) v[u] = tt[u] < rows ? g[index[tt[u]] * quads + cc[u]] : uint4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int u = 0; u < kResampleGatherBatch; u++)
          if (tt[u] < rows) { /* the row in LDS keeps the odd-word stride: four word stores, none past the row's K/2 words */
            uint32_t *const dst = row_words + tt[u] * stride_words + 4 * cc[u];
            const uint32_t left = half - 4 * cc[u]; /* > 0 but for a piece that is padding alone */
            if (4 * cc[u] < half) dst[0] = v[u].x;
            if (4 * cc[u] < half && left > 1) dst[1] = v[u].y;
            if (4 * cc[u] < half && left > 2) dst[2] = v[u].z;
            if (4 * cc[u] < half && left > 3) dst[3] = v[u].w;
          }
      }
      __syncthreads();
      if (mine) emit(n, resample_dot(span_words, row_words + t_mine * stride_words, at.front + (i - at.i0), half));
    }
    i += di;
    p += dp;
    if (p >= d.L) {
      p -= d.L;
      i += 1;
    }
  }
}

/* the tile of a wide resampler: `index` is the phase index, `round` words behind bank and span */
struct ResampleWide {
  uint32_t round;
  template <class Emit>
  __device__ __forceinline__ void operator()(const ResampleRowsArgs &a, uint32_t *bank_words, uint32_t *span_words, uint32_t &staged,
                                             uint64_t row, uint32_t bank, uint32_t shift, uint32_t n0, uint32_t n_end, Emit emit) const
  {
    const ResampleBankDesc d = a.banks[bank];
    if (resample_bank_resident(d.L, d.K)) {
      resample_tile(a, bank_words, span_words, staged, row, bank, shift, n0, n_end, emit);
    } else {
      staged = ~0u; /* the rows go where a whole bank would */
      resample_tile_gathered(a, d, round, bank_words, span_words, span_words + a.span_elements / 2, row, shift, n0, n_end, emit);
    }
  }
};

template <int ST>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_wide_kernel(ResampleMixArgs m)
{
  resample_rows_body<ST>(m.r, ResampleWide{m.round});
}

template <int ST, bool ADD>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_gain_wide_kernel(ResampleMixArgs m)
{
  resample_rows_gain_body<ST, ADD>(m, ResampleWide{m.round});
}

template <int ST>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_stats_wide_kernel(ResampleMixArgs m)
{
  resample_rows_stats_body<ST>(m, ResampleWide{m.round});
}

template <class Kernel>
static bool launch_wide(Kernel kernel, const ResampleMixArgs &m, uint32_t lds_bytes, hipStream_t stream)
{
  if (lds_bytes > 65536u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return false;
  AAD_LAUNCH(kernel, dim3(resample_grid(m.r)), dim3(kResampleThreads), lds_bytes, stream, m);
  return true;
}

bool launch_resample_rows_wide(const ResampleMixArgs &m, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream)
{
  switch (sample_type) {
    case AAD_HIP_SAMPLE_INT16: return launch_wide(&resample_rows_wide_kernel<AAD_HIP_SAMPLE_INT16>, m, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT32: return launch_wide(&resample_rows_wide_kernel<AAD_HIP_SAMPLE_FLOAT32>, m, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT16: return launch_wide(&resample_rows_wide_kernel<AAD_HIP_SAMPLE_FLOAT16>, m, lds_bytes, stream);
    default: return launch_wide(&resample_rows_wide_kernel<AAD_HIP_SAMPLE_BFLOAT16>, m, lds_bytes, stream);
  }
}

bool launch_resample_rows_gain_wide(const ResampleMixArgs &m, int32_t sample_type, bool add, uint32_t lds_bytes, hipStream_t stream)
{
  switch (sample_type) {
    case AAD_HIP_SAMPLE_FLOAT32:
      return add ? launch_wide(&resample_rows_gain_wide_kernel<AAD_HIP_SAMPLE_FLOAT32, true>, m, lds_bytes, stream)
                 : launch_wide(&resample_rows_gain_wide_kernel<AAD_HIP_SAMPLE_FLOAT32, false>, m, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT16:
      return add ? launch_wide(&resample_rows_gain_wide_kernel<AAD_HIP_SAMPLE_FLOAT16, true>, m, lds_bytes, stream)
                 : launch_wide(&resample_rows_gain_wide_kernel<AAD_HIP_SAMPLE_FLOAT16, false>, m, lds_bytes, stream);
    default:
      return add ? launch_wide(&resample_rows_gain_wide_kernel<AAD_HIP_SAMPLE_BFLOAT16, true>, m, lds_bytes, stream)
                 : launch_wide(&resample_rows_gain_wide_kernel<AAD_HIP_SAMPLE_BFLOAT16, false>, m, lds_bytes, stream);
  }
}

bool launch_resample_rows_stats_wide(const ResampleMixArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream)
{
  ResampleMixArgs m = a;
  const uint32_t scratch = resample_stats_scratch_offset(lds_bytes);
  m.scratch_words = scratch / 4;
  lds_bytes = scratch + kResampleStatsScratchBytes;
  if (m.r.out == nullptr) return launch_wide(&resample_rows_stats_wide_kernel<kResampleNoRows>, m, lds_bytes, stream);
  switch (sample_type) {
    case AAD_HIP_SAMPLE_INT16: return launch_wide(&resample_rows_stats_wide_kernel<AAD_HIP_SAMPLE_INT16>, m, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT32: return launch_wide(&resample_rows_stats_wide_kernel<AAD_HIP_SAMPLE_FLOAT32>, m, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT16: return launch_wide(&resample_rows_stats_wide_kernel<AAD_HIP_SAMPLE_FLOAT16>, m, lds_bytes, stream);
    default: return launch_wide(&resample_rows_stats_wide_kernel<AAD_HIP_SAMPLE_BFLOAT16>, m, lds_bytes, stream);
  }
}

} /* namespace aad */
