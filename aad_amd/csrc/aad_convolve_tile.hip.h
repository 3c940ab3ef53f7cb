/* aad_convolve_tile.hip.h - the bodies of the convolve stage's FIR kernels (aad_convolve.hip instantiates them).  Device code only.
 *
 * convolve_tile  One workgroup of four waves per (window, channel row, tile of kConvolveTile = 4096 outputs).  The exact sum
 *   acc[n] = sum_k h[k] x[...] of 16-bit values is four products of signed bytes on the matrix cores, int32 accumulators
 *   (__builtin_amdgcn_mfma_i32_16x16x64_i8):  x = 256 xh + xl + 128 and h = 256 hh + hl (convolve_split_sample, convolve_split), so
 *     acc = 65536 P(xh, hh) + 256 (P(xh, hl) + P(xl, hh)) + P(xl, hl) + 128 sum h,
 *   each P below K 2^14 <= 2^29 in magnitude - the middle pair shares an accumulator - and the combination in 64-bit integers in
 *   the epilogue, with the response's constant (ResponseDesc::bias).
 *   A block of 256 outputs is one 16 x 16 accumulator tile (aad_convolve.h, convolve_build_planes): A's rows are runs of the source
 *   span 16 bytes apart, in an xh plane and an xl plane in LDS that the staging loop writes - a frame the row does not have is x = 0
 *   like any other zero - and B is the response's Hankel matrix, whose byte planes the host built in operand order: a lane's
 *   fragment of a k-step is one aligned 16-byte load from global memory, the loads of step s + 1 in flight under step s.  Lane l
 *   holds A[row l & 15][16 (l >> 4) + e] and B[16 (l >> 4) + e][col l & 15], e < 16: the two operands share the order of the sum
 *   index whatever it is, so only row, column and the group of 16 matter.  A wave keeps kConvolveWaveBlocks blocks' accumulators -
 *   blocks wave, wave + 4, ... of the tile, so that a short tile spreads over the waves - and uses a fragment of B for all of them.
 *   Row i of a block's A holds the outputs 16 (4 (i & 3) + (i >> 2)) ...: register r of the accumulator (row 4 (l >> 4) + r,
 *   column l & 15) is then output 64 r + l of the block, and a wave's store is 64 adjacent elements.
 *   K is walked in pieces of kConvolvePieceSteps k-steps (4096 taps): the planes hold the tile's outputs and one piece's taps,
 *   16 KB together whatever K is, and are staged again for the next piece.
 *   Every LDS read lies inside what the piece staged (kConvolveSpan), every load of B inside the response's steps, and a source
 *   element is read only when 0 <= j < source_frames. */
#ifndef AAD_CONVOLVE_TILE_HIP_H
#define AAD_CONVOLVE_TILE_HIP_H

#include "aad_convolve.hip.h"
#include "aad_resample_tile.hip.h"

namespace aad {
namespace convolve {

typedef int i32x4 __attribute__((ext_vector_type(4)));

/* the sample type's element of an exact sum (aad_convolve.h) */
template <int ST>
__device__ __forceinline__ typename ResampleOut<ST>::T element(int64_t acc, uint32_t q)
{
  if constexpr (ST == AAD_HIP_SAMPLE_INT16) return convolve_int16(acc, q);
  else return ResampleFloat<ST>::narrow(convolve_float(acc, q));
}

/* the k-steps of one staged piece for the wave's first NB blocks */
template <int NB>
__device__ __forceinline__ void piece_steps(i32x4 (&acc)[kConvolveWaveBlocks][3], const uint8_t *xh, const uint8_t *xl,
                                            const i32x4 *b, uint32_t nsteps, uint32_t at)
{
  i32x4 bh = b[0], bl = b[64];
  for (uint32_t s = 0; s < nsteps; s++) {
    const uint32_t next = s + 1 < nsteps ? s + 1 : s; /* the last step loads itself again: no branch, no load past the response */
    const i32x4 nh = b[128 * next], nl = b[128 * next + 64];
    i32x4 ah[NB], al[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) {
      const uint32_t e = at + 4 * kConvolveBlock * k + kConvolveStepTaps * s;
      ah[k] = *reinterpret_cast<const i32x4 *>(xh + e);
      al[k] = *reinterpret_cast<const i32x4 *>(xl + e);
    }
#pragma unroll
    for (int k = 0; k < NB; k++) acc[k][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[k], bh, acc[k][0], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) acc[k][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[k], bl, acc[k][1], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) acc[k][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[k], bl, acc[k][2], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) acc[k][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[k], bh, acc[k][1], 0, 0, 0);
    bh = nh;
    bl = nl;
  }
}

/* One tile of one row with response d, for every FIR kernel: acc of the outputs n0 <= n < n_end, each handed to emit(n, acc).
 * Uniform over the workgroup. */
template <class Emit>
__device__ __forceinline__ void convolve_tile(const RowsArgs &a, uint32_t *lds, const ResponseDesc &d, uint64_t row, uint32_t shift,
                                              uint32_t n0, uint32_t n_end, Emit emit)
{
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t *const xh_words = lds, *const xl_words = lds + kConvolveSpan / 4;
  const uint32_t blocks = (n_end - n0 + kConvolveBlock - 1) / kConvolveBlock; /* of the tile, 1 ... 16 */
  const uint32_t mine = blocks > wave ? (blocks - wave + 3) / 4 : 0;         /* of this wave: blocks wave, wave + 4, ... */
  const int16_t *const src_row = a.src + row * a.source_frames;
  /* element 0 of the span: the first output's first tap in the order of the reversed response */
  const int64_t j0 = (int64_t)shift - (int64_t)(d.K - 1 - d.delay) + (int64_t)n0;
  const uint32_t at = kConvolveBlock * wave + 16 * (4 * (lane & 3u) + ((lane & 15u) >> 2) + (lane >> 4));
  const i32x4 *const planes = reinterpret_cast<const i32x4 *>(a.planes + d.offset) + lane;
  i32x4 acc[kConvolveWaveBlocks][3] = {};
  for (uint32_t p0 = 0; p0 < d.steps; p0 += kConvolvePieceSteps) {
    const uint32_t nsteps = d.steps - p0 < kConvolvePieceSteps ? d.steps - p0 : kConvolvePieceSteps;
    const uint32_t words = (kConvolveBlock * blocks + kConvolveStepTaps * nsteps) / 4; /* <= kConvolveSpan / 4 */
    const int64_t jp = j0 + (int64_t)kConvolveStepTaps * p0;
    __syncthreads(); /* the previous piece's, or the previous item's, reads are done */
    for (uint32_t wi = tid; wi < words; wi += kConvolveThreads) {
      const int64_t j = jp + 4 * (int64_t)wi;
      uint32_t hi = 0, lo = 0x80808080u;
      if (j + 3 >= 0 && j < (int64_t)a.source_frames) {
        hi = lo = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int16_t x = j + e >= 0 && j + e < (int64_t)a.source_frames ? src_row[j + e] : (int16_t)0;
          const ConvolveBytes b = convolve_split_sample(x);
          hi |= (uint32_t)(uint8_t)b.hh << (8 * e);
          lo |= (uint32_t)(uint8_t)b.hl << (8 * e);
        }
      }
      xh_words[wi] = hi;
      xl_words[wi] = lo;
    }
    __syncthreads();
    const uint8_t *const xh = reinterpret_cast<const uint8_t *>(xh_words), *const xl = reinterpret_cast<const uint8_t *>(xl_words);
    const i32x4 *const b = planes + 128 * p0;
    switch (mine) {
      case 4: piece_steps<4>(acc, xh, xl, b, nsteps, at); break;
      case 3: piece_steps<3>(acc, xh, xl, b, nsteps, at); break;
      case 2: piece_steps<2>(acc, xh, xl, b, nsteps, at); break;
      case 1: piece_steps<1>(acc, xh, xl, b, nsteps, at); break;
      default: break;
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < kConvolveWaveBlocks; k++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const uint32_t n = n0 + kConvolveBlock * (wave + 4 * k) + 64 * r + lane;
      if (k < mine && n < n_end)
        emit(n, (int64_t)acc[k][0][r] * 65536 + (int64_t)acc[k][1][r] * 256 + (int64_t)acc[k][2][r] + d.bias);
    }
  }
}

static_assert(kConvolveWaveBlocks == 4 && kConvolveThreads == 256, "the waves' blocks: wave + 4 k, k < 4");
static_assert((kConvolveTile - kConvolveBlock) + 16 * (15 + 3) + kConvolveStepTaps * (kConvolvePieceSteps - 1) + 16 <= kConvolveSpan,
              "the last fragment read of a piece");

/* ---- plain rows (AADHip_ConvolverRun) ------------------------------------------------------------------------------------------- */

template <int ST>
__device__ __forceinline__ void rows_body(const RowsArgs &a)
{
  typedef typename ResampleOut<ST>::T T;
  __shared__ __attribute__((aligned(16))) uint32_t lds[2 * kConvolveSpan / 4];
  const uint32_t tid = threadIdx.x;
  const uint64_t items = a.rows * a.tiles;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.tiles, w = row / a.channels;
    const uint32_t n0 = (uint32_t)(item - row * a.tiles) * kConvolveTile;
    const uint32_t n_end = a.frames - n0 < kConvolveTile ? a.frames : n0 + kConvolveTile;
    T *const out = static_cast<T *>(a.out) + row * a.frames;
    const uint32_t response = __builtin_amdgcn_readfirstlane(a.lanes[w].response);
    if (response >= a.num_responses) { /* no response: +0 */
      for (uint32_t n = n0 + tid; n < n_end; n += kConvolveThreads) out[n] = (T)0;
      continue;
    }
    const uint32_t shift = __builtin_amdgcn_readfirstlane(a.lanes[w].shift);
    const ResponseDesc d = a.responses[response];
    convolve_tile(a, lds, d, row, shift, n0, n_end, [&](uint32_t n, int64_t acc) { out[n] = element<ST>(acc, d.q); });
  }
}

/* ---- rows with gain and spans (AADHip_ConvolverRunGain) ------------------------------------------------------------------------- */

/* Items as the plain kernel's: the tile's crop indices n < Le go through the FIR and land at o + n; under STORE the workgroup also
 * writes +0 to the row elements of its tile that lie outside the span (window_fill_tile with the tile as the block), so every
 * element of a row is written exactly once, by one thread - resample_rows_gain_body's scheme with its writer, resample_gain_put. */
template <int ST, bool ADD>
__device__ __forceinline__ void rows_gain_body(const GainArgs &m)
{
  typedef typename ResampleOut<ST>::T T;
  const RowsArgs &a = m.r;
  __shared__ __attribute__((aligned(16))) uint32_t lds[2 * kConvolveSpan / 4];
  const uint32_t tid = threadIdx.x;
  const uint64_t items = a.rows * a.tiles;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.tiles, w = row / a.channels;
    const uint32_t tile_index = (uint32_t)(item - row * a.tiles), n0 = tile_index * kConvolveTile;
    const ResampleSpan s = resample_span(m.spans, w, a.frames);
    T *const out = static_cast<T *>(a.out) + row * a.frames;
    if (!ADD) {
      const WindowFillTile fill = window_fill_tile(tile_index, kConvolveTile, 0, a.frames, s.o, s.le);
      for (int piece = 0; piece < 2; piece++)
        for (int64_t e = fill.lo[piece] + tid; e < fill.hi[piece]; e += kConvolveThreads) out[e] = (T)0;
    }
    if (n0 >= s.le) continue;
    const uint32_t n_end = s.le - n0 < kConvolveTile ? s.le : n0 + kConvolveTile;
    T *const dst = out + s.o; /* o < T: Le > 0 */
    const float g = m.gain != nullptr ? m.gain[w] : 1.0f;
    const uint32_t response = __builtin_amdgcn_readfirstlane(a.lanes[w].response);
    if (response >= a.num_responses) { /* no response: f = +0 */
      for (uint32_t n = n0 + tid; n < n_end; n += kConvolveThreads) resample_gain_put<ST, ADD>(dst + n, g, 0.0f);
      continue;
    }
    const uint32_t shift = __builtin_amdgcn_readfirstlane(a.lanes[w].shift);
    const ResponseDesc d = a.responses[response];
    convolve_tile(a, lds, d, row, shift, n0, n_end,
                  [&](uint32_t n, int64_t acc) { resample_gain_put<ST, ADD>(dst + n, g, convolve_float(acc, d.q)); });
  }
}

/* the grid of every FIR launch: one workgroup per item up to 2^20, the kernels' item loop takes the rest */
inline uint32_t grid(const RowsArgs &a)
{
  const uint64_t items = a.rows * a.tiles;
  return items < (1u << 20) ? (uint32_t)items : (1u << 20);
}

} /* namespace convolve */
} /* namespace aad */

#endif /* AAD_CONVOLVE_TILE_HIP_H */
