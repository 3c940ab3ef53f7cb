/* aad_spectrogram_rows.hip.h - the device code of the spectrogram stage, shared by its translation units: aad_spectrogram.hip
 * (namespace aad::spectrum, rows read as they lie) and aad_spectrogram_mix.hip (aad::spectrum_mix, two row batches summed at gains
 * while staged).  What differs between them is how a sample of the tile comes to be - a STAGER, below - and nothing else: the
 * k-step loop, the epilogue and the filterbank pass exist once, here.
 *
 * rows_body<MEL>  One workgroup of four waves per (row, tile of up to kSpectrumTileFrames frames); items past 2^20
 *   workgroups go through the item loop.  The framed real DFT is convolve_tile's arithmetic (aad_convolve_tile.hip.h) with a dense
 *   matrix: the exact sums Re[f][k], Im[f][k] of 16-bit values are four products of signed bytes on the matrix cores
 *   (__builtin_amdgcn_mfma_i32_16x16x64_i8), x = 256 xh + xl + 128 and c = 256 ch + cl, so
 *     sum = 65536 P(xh, ch) + 256 (P(xh, cl) + P(xl, ch)) + P(xl, cl) + 128 sum c,
 *   combined exactly, in double, with the column's constant (spectrum_column_constants, spectrum_element).
 *   The tile's samples are staged into an xh and an xl plane in LDS, frame i of the tile at element i * pitch
 *   (spectrum_geometry): a hop that is a multiple of 16 stages the tile's span of the row once, any other hop frame by frame.  A
 *   block of 16 frames is the 16 rows of A; lane l holds A[frame l & 15][64 s + 16 (l >> 4) + e] and B[the same t][column
 *   l & 15], e < 16 - one aligned 16-byte read of LDS and one aligned 16-byte load of the planes the host built in that order
 *   (spectrum_build_planes), the loads of step s + 1 in flight under step s.  A wave keeps kSpectrumWaveBlocks blocks - blocks
 *   wave, wave + 4, ... - and uses a fragment of B for all of them: 24 accumulator registers a block, Re and Im with three
 *   accumulators each.
 *   Column tile pairs (Re, Im of bins 16 c ... 16 c + 15) run in ascending order outside, k-steps inside.  After a pair, register
 *   r of a lane is frame 4 (l >> 4) + r of the block and bin 16 c + (l & 15), Re and Im both: P needs no cross-lane move.
 *   MEL false: P is stored straight from the lanes.  MEL true: the pair's powers go through a hand-off buffer in LDS to one
 *   thread per frame, which runs the filters that touch the pair's bins (spectrum_tile_lists) in the definition's order - a filter
 *   that began in an earlier pair continues from its element of `out`, which only this thread ever reads or writes - so that no
 *   frames x B powers are kept anywhere.
 *   A stager's sample is asked for only at an index below the row's `frames`; every LDS read lies inside what the item staged
 *   ((16 blocks - 1) pitch + 64 steps elements a plane, at most g.plane_elements); every load of B lies inside the planes
 *   (2 pairs x steps steps).  The float arithmetic is __fmul_rn / __fadd_rn, and the units compile with -ffp-contract=off.
 *
 * A stager: `row(r)` gives the state of row r of the run, made once per item, and its `sample(j)`, j < frames, the int16 value
 * that element j of the row stands for. */
#ifndef AAD_SPECTROGRAM_ROWS_HIP_H
#define AAD_SPECTROGRAM_ROWS_HIP_H

#include "aad_spectrogram.hip.h"

#include "../../include/aad_hip.h"
#include "aad_launch.h"

namespace aad {
namespace spectrum {

typedef int i32x4 __attribute__((ext_vector_type(4)));

/* the rows as they lie: AADHip_SpectrogramRun */
struct PlainStager {
  struct Row {
    const int16_t *src;
    __device__ __forceinline__ int16_t sample(uint64_t j) const { return src[j]; }
  };
  const Args &a;
  __device__ __forceinline__ Row row(uint64_t r) const { return Row{a.rows + r * a.row_pitch}; }
};

/* the k-steps of one column tile pair for the wave's first NB blocks; b: the lane's fragment of the Re tile's step 0 */
template <int NB>
__device__ __forceinline__ void pair_steps(i32x4 (&re)[kSpectrumWaveBlocks][3], i32x4 (&im)[kSpectrumWaveBlocks][3], const uint8_t *xh,
                                           const uint8_t *xl, const i32x4 *b, uint32_t steps, uint32_t at, uint32_t block_stride)
{
  const i32x4 *const bi = b + 128 * steps; /* the Im tile */
  i32x4 rh = b[0], rl = b[64], ih = bi[0], il = bi[64];
  for (uint32_t s = 0; s < steps; s++) {
    const uint32_t next = s + 1 < steps ? s + 1 : s; /* the last step loads itself again: no branch, no load past the tile */
    const i32x4 nrh = b[128 * next], nrl = b[128 * next + 64], nih = bi[128 * next], nil = bi[128 * next + 64];
    i32x4 ah[NB], al[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) {
      const uint32_t e = at + block_stride * k + kConvolveStepTaps * s;
      ah[k] = *reinterpret_cast<const i32x4 *>(xh + e);
      al[k] = *reinterpret_cast<const i32x4 *>(xl + e);
    }
#pragma unroll
    for (int k = 0; k < NB; k++) re[k][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[k], rh, re[k][0], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) im[k][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[k], ih, im[k][0], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) re[k][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[k], rl, re[k][1], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) im[k][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah[k], il, im[k][1], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) re[k][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[k], rl, re[k][2], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) im[k][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[k], il, im[k][2], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) re[k][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[k], rh, re[k][1], 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; k++) im[k][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al[k], ih, im[k][1], 0, 0, 0);
    rh = nrh;
    rl = nrl;
    ih = nih;
    il = nil;
  }
}

template <bool MEL, class Stager>
__device__ __forceinline__ void rows_body(const Args &a, const Stager &stager)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t spectrum_lds[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t plane_words = (a.g.plane_elements + 15u) / 16u * 4u;
  uint32_t *const xh_words = spectrum_lds, *const xl_words = spectrum_lds + plane_words;
  float *const exchange = reinterpret_cast<float *>(spectrum_lds + 2 * plane_words);
  const uint8_t *const xh = reinterpret_cast<const uint8_t *>(xh_words), *const xl = reinterpret_cast<const uint8_t *>(xl_words);
  const uint32_t pitch = a.g.pitch, step_elements = kConvolveStepTaps * a.steps;
  const uint32_t at = (16 * wave + (lane & 15u)) * pitch + 16 * (lane >> 4), block_stride = 64 * pitch;
  const i32x4 *const planes = reinterpret_cast<const i32x4 *>(a.planes) + lane;
  const uint64_t items = a.num_rows * a.tiles;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.tiles;
    const uint32_t f0 = (uint32_t)(item - row * a.tiles) * a.g.tile_frames;
    const uint32_t nf = a.num_frames - f0 < a.g.tile_frames ? a.num_frames - f0 : a.g.tile_frames; /* frames of the tile */
    const uint32_t blocks = (nf + 15) / 16;                                                        /* 1 ... 16 */
    const uint32_t mine = blocks > wave ? (blocks - wave + 3) / 4 : 0; /* of this wave: blocks wave, wave + 4, ... */
    const typename Stager::Row src = stager.row(row);
    const uint32_t words = ((16 * blocks - 1) * pitch + step_elements) / 4; /* <= g.plane_elements / 4 */
    __syncthreads(); /* the previous item's reads are done */
    for (uint32_t wi = tid; wi < words; wi += kSpectrumThreads) {
      /* element 4 wi of the plane is sample j of the row: the span from frame f0 on, or sample `off` of the tile's frame fl */
      const uint32_t fl = a.g.frame_major ? 4 * wi / pitch : 0;
      const uint64_t j = (uint64_t)(f0 + fl) * a.hop + (4 * wi - fl * pitch);
      uint32_t hi = 0, lo = 0x80808080u;
      if (j < a.frames) {
        hi = lo = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int16_t x = j + e < a.frames ? src.sample(j + e) : (int16_t)0;
          const ConvolveBytes b = convolve_split_sample(x);
          hi |= (uint32_t)(uint8_t)b.hh << (8 * e);
          lo |= (uint32_t)(uint8_t)b.hl << (8 * e);
        }
      }
      xh_words[wi] = hi;
      xl_words[wi] = lo;
    }
    __syncthreads();
    for (uint32_t c = 0; c < a.pairs; c++) {
      i32x4 re[kSpectrumWaveBlocks][3] = {}, im[kSpectrumWaveBlocks][3] = {};
      const i32x4 *const b = planes + (size_t)128 * (2 * c) * a.steps;
      switch (mine) {
        case 4: pair_steps<4>(re, im, xh, xl, b, a.steps, at, block_stride); break;
        case 3: pair_steps<3>(re, im, xh, xl, b, a.steps, at, block_stride); break;
        case 2: pair_steps<2>(re, im, xh, xl, b, a.steps, at, block_stride); break;
        case 1: pair_steps<1>(re, im, xh, xl, b, a.steps, at, block_stride); break;
        default: break;
      }
      const uint32_t bin = 16 * c + (lane & 15u);
      const double scale = spectrum_scale(a.q);
      const double re_const = (double)a.consts[bin] * scale, im_const = (double)a.consts[16 * a.pairs + bin] * scale;
#pragma unroll
      for (uint32_t k = 0; k < kSpectrumWaveBlocks; k++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const uint32_t fl = 16 * (wave + 4 * k) + 4 * (lane >> 4) + r;
          if (k < mine && fl < nf) {
            const float p = spectrum_power(spectrum_element(re[k][0][r], re[k][1][r], re[k][2][r], re_const, scale),
                                           spectrum_element(im[k][0][r], im[k][1][r], im[k][2][r], im_const, scale));
            if constexpr (MEL) exchange[kSpectrumExchangePitch * fl + (lane & 15u)] = p; /* a bin past B: its columns are zero */
            else if (bin < a.bins) a.out[(row * a.num_frames + f0 + fl) * a.bins + bin] = p;
          }
        }
      }
      if constexpr (MEL) {
        __syncthreads();
        if (tid < nf) {
          float *const e_row = a.out + (row * a.num_frames + f0 + tid) * a.num_filters;
          const float *const p_row = exchange + kSpectrumExchangePitch * tid;
          const uint32_t k0 = 16 * c, list_end = a.tile_first[c + 1];
          for (uint32_t i = a.tile_first[c]; i < list_end; i++) {
            const uint32_t j = a.tile_list[i];
            const SpectrumBand band = a.bands[j];
            const uint32_t ka = band.lo > k0 ? band.lo : k0, kb = band.hi < k0 + 15 ? band.hi : k0 + 15;
            float e = band.lo >= k0 ? 0.0f : e_row[j]; /* the filter begins here (an all-zero one: lo = B, no bin), or goes on */
            for (uint32_t k = ka; k <= kb; k++) e = __fadd_rn(e, __fmul_rn(a.weights[band.offset + (k - band.lo)], p_row[k - k0]));
            e_row[j] = e;
          }
        }
        __syncthreads(); /* the buffer is free for the next pair */
      }
    }
  }
}

/* the launch of a unit's kernel over a run's items, with the run's LDS; false: the device refuses it (spectrum_lds_bytes) */
template <class KernelArgs>
static bool launch_rows(void (*kernel)(KernelArgs), const KernelArgs &k, const Args &a, bool mel, hipStream_t stream)
{
  const uint32_t lds_bytes = spectrum_lds_bytes(a.g, mel) + 64; /* the planes end on 16-byte boundaries */
  if (lds_bytes > 65536u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess)
    return false;
  const uint64_t items = a.num_rows * a.tiles;
  AAD_LAUNCH(kernel, dim3(items < (1u << 20) ? (uint32_t)items : (1u << 20)), dim3(kSpectrumThreads), lds_bytes, stream, k);
  return true;
}

} /* namespace spectrum */
} /* namespace aad */

#endif /* AAD_SPECTROGRAM_ROWS_HIP_H */
