/* aad_resample.hip - translation unit of the resample stage's two kernels (aad_resample.hip.h).
 *
 * resample_resolve_kernel  one thread per window, in front of the window decode: resample_resolve (aad_resample.h) gives the source
 *   window - the window moved K/2 - 1 frames to the front, or to frame 0 - and the lane record {bank, shift} the FIR kernel reads.
 *
 * resample_rows_kernel<ST>  behind the window decode, which has written the int16 source batch.  One workgroup per (window, channel
 *   row, tile of 1024 outputs); thread tid produces outputs tile + tid + 256 j, so a wave's stores are 64 adjacent elements.  The
 *   bank of the row's window (uniform per workgroup) goes into LDS, phase p's K taps at p * stride int16 (resample_lds_stride: an
 *   odd number of words, adjacent outputs read different phases), and the span of the source row the tile reads behind it, zero
 *   where the row has no frame.  The span starts on a 4-byte boundary of the source buffer, so the row is read in whole words.
 *   Output n = (i, p): acc = sum_k h[p][k] x[i + k], two taps per v_dot2: the coefficient pair is one word of the phase's row, the
 *   sample pair one word of the span, or - for a thread whose first sample sits at an odd element - the middle of two words, one
 *   v_alignbit; four pairs a round, their eight LDS reads issued together.  int16 x int16 into int32 is exact: sum |h| <= 65535
 *   per phase.  Then the sample type's conversion
 *   (include/aad_hip.h "resample") and one ordinary store.
 *   A workgroup that takes a further item (grids past 2^20 workgroups) keeps its bank when the next row's is the same. */
#include "aad_resample.hip.h"
#include "aad_launch.h"

namespace aad {

__global__ void __launch_bounds__(256) resample_resolve_kernel(ResampleResolveArgs a)
{
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.num_windows) return;
  const ResampleResolved r = resample_resolve(a.windows[2 * w], a.windows[2 * w + 1], a.variant != nullptr ? a.variant[w] : 0,
                                              a.num_streams, a.variants, a.select, a.lead);
  a.source_windows[2 * w] = r.stream;
  a.source_windows[2 * w + 1] = r.src_first;
  a.lanes[w] = r.lane;
}

void launch_resample_resolve(const ResampleResolveArgs &a, hipStream_t stream)
{
  AAD_LAUNCH(resample_resolve_kernel, dim3((uint32_t)((a.num_windows + 255) / 256)), dim3(256), 0, stream, a);
}

typedef short resample_i16x2 __attribute__((ext_vector_type(2)));

template <int ST>
struct ResampleOut;
template <>
struct ResampleOut<AAD_HIP_SAMPLE_INT16> {
  typedef int16_t T;
  __device__ __forceinline__ static T of(int32_t acc)
  {
    const int32_t v = (acc + 8192) >> 14; /* floor: |acc| + 8192 < 2^31 */
    return (T)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
  }
};
template <>
struct ResampleOut<AAD_HIP_SAMPLE_FLOAT32> {
  typedef float T;
  __device__ __forceinline__ static T of(int32_t acc) { return (float)acc * 0x1p-29f; } /* one rounding, then an exact scale */
};
template <>
struct ResampleOut<AAD_HIP_SAMPLE_FLOAT16> {
  typedef uint16_t T;
  __device__ __forceinline__ static T of(int32_t acc) { return __builtin_bit_cast(uint16_t, (_Float16)((float)acc * 0x1p-29f)); }
};
template <>
struct ResampleOut<AAD_HIP_SAMPLE_BFLOAT16> {
  typedef uint16_t T;
  __device__ __forceinline__ static T of(int32_t acc) { return __builtin_bit_cast(uint16_t, (__bf16)((float)acc * 0x1p-29f)); }
};

template <int ST>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_kernel(ResampleRowsArgs a)
{
  typedef typename ResampleOut<ST>::T T;
  extern __shared__ __attribute__((aligned(16))) uint32_t resample_lds[];
  uint32_t *const bank_words = resample_lds;
  uint32_t *const span_words = resample_lds + a.bank_elements / 2;
  const uint32_t tid = threadIdx.x;
  const uint64_t items = a.rows * a.tiles;
  uint32_t staged = ~0u;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.tiles, w = row / a.channels;
    const uint32_t n0 = (uint32_t)(item - row * a.tiles) * kResampleTile;
    const uint32_t n_end = a.frames - n0 < kResampleTile ? a.frames : n0 + kResampleTile;
    T *const out = static_cast<T *>(a.out) + row * a.frames;
    const uint32_t bank = __builtin_amdgcn_readfirstlane(a.lanes[w].bank);
    if (bank >= a.num_banks) { /* no bank: +0 */
      for (uint32_t n = n0 + tid; n < n_end; n += kResampleThreads) out[n] = (T)0;
      continue;
    }
    const uint32_t shift = __builtin_amdgcn_readfirstlane(a.lanes[w].shift);
    const ResampleBankDesc d = a.banks[bank];
    const uint32_t half = d.K / 2, stride_words = resample_lds_stride(d.K) / 2;
    __syncthreads(); /* the previous item's reads are done */
    if (staged != bank) {
      const uint32_t *g = reinterpret_cast<const uint32_t *>(a.coefficients + d.offset);
      for (uint32_t idx = tid; idx < d.L * half; idx += kResampleThreads) {
        const uint32_t p = idx / half;
        bank_words[p * stride_words + (idx - p * half)] = g[idx];
      }
      staged = bank;
    }
    /* the span: element e is the source row's frame jb + e, jb on a 4-byte boundary of the buffer */
    const uint32_t i0 = (uint32_t)(((uint64_t)n0 * d.M) / d.L);
    const uint32_t i_last = (uint32_t)(((uint64_t)(n_end - 1) * d.M) / d.L);
    const uint64_t row_base = row * a.source_frames;
    int64_t jb = (int64_t)shift + (int64_t)i0 - (int64_t)(half - 1);
    const uint32_t front = (uint32_t)(((reinterpret_cast<uintptr_t>(a.src) >> 1) + row_base + (uint64_t)jb) & 1u);
    jb -= front;
    uint32_t words = (front + (i_last - i0) + d.K + 2 + 1) / 2; /* the last output's last tap, and the word read behind it */
    if (words > a.span_elements / 2) words = a.span_elements / 2;
    const int16_t *const src_row = a.src + row_base;
    for (uint32_t wi = tid; wi < words; wi += kResampleThreads) {
      const int64_t j = jb + 2 * (int64_t)wi;
      uint32_t v;
      if (j >= 0 && j + 1 < (int64_t)a.source_frames) {
        v = *reinterpret_cast<const uint32_t *>(src_row + j);
      } else {
        const uint32_t lo = j >= 0 && j < (int64_t)a.source_frames ? (uint16_t)src_row[j] : 0u;
        const uint32_t hi = j + 1 >= 0 && j + 1 < (int64_t)a.source_frames ? (uint16_t)src_row[j + 1] : 0u;
        v = lo | (hi << 16);
      }
      span_words[wi] = v;
    }
    __syncthreads();
    /* (256 M) div / mod L: taken only by outputs tid + 256 j, j >= 1, which exist when T > 256 and then M < 2^23 */
    const uint32_t step = kResampleThreads * d.M, di = step / d.L, dp = step - di * d.L;
    uint32_t n = n0 + tid;
    const uint32_t nm = n * d.M;
    uint32_t i = nm / d.L, p = nm - i * d.L;
#pragma unroll 1
    for (uint32_t j = 0; j < kResamplePerThread && n < n_end; j++, n += kResampleThreads) {
      const uint32_t e0 = front + (i - i0);
      const uint32_t *x = span_words + (e0 >> 1);
      const uint32_t *h = bank_words + p * stride_words;
      const uint32_t odd = (e0 & 1u) * 16u;
      int32_t acc = 0;
      uint32_t lo = x[0];
      uint32_t q = 0;
      for (; q + 4 <= half; q += 4) { /* eight reads in flight, then four dot products: one LDS latency per eight taps */
        const uint32_t x1 = x[q + 1], x2 = x[q + 2], x3 = x[q + 3], x4 = x[q + 4];
        const uint32_t h0 = h[q], h1 = h[q + 1], h2 = h[q + 2], h3 = h[q + 3];
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_i16x2, __builtin_amdgcn_alignbit(x1, lo, odd)),
                                     __builtin_bit_cast(resample_i16x2, h0), acc, false);
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_i16x2, __builtin_amdgcn_alignbit(x2, x1, odd)),
                                     __builtin_bit_cast(resample_i16x2, h1), acc, false);
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_i16x2, __builtin_amdgcn_alignbit(x3, x2, odd)),
                                     __builtin_bit_cast(resample_i16x2, h2), acc, false);
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_i16x2, __builtin_amdgcn_alignbit(x4, x3, odd)),
                                     __builtin_bit_cast(resample_i16x2, h3), acc, false);
        lo = x4;
      }
      for (; q < half; q++) {
        const uint32_t hi = x[q + 1];
        const uint32_t pair = __builtin_amdgcn_alignbit(hi, lo, odd);
        acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_i16x2, pair), __builtin_bit_cast(resample_i16x2, h[q]), acc, false);
        lo = hi;
      }
      out[n] = ResampleOut<ST>::of(acc);
      i += di;
      p += dp;
      if (p >= d.L) {
        p -= d.L;
        i += 1;
      }
    }
  }
}

template <int ST>
static bool launch_type(const ResampleRowsArgs &a, uint32_t lds_bytes, hipStream_t stream)
{
  if (lds_bytes > 65536u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(&resample_rows_kernel<ST>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_bytes) != hipSuccess)
    return false;
  const uint64_t items = a.rows * a.tiles;
  const uint32_t grid = items < (1u << 20) ? (uint32_t)items : (1u << 20);
  AAD_LAUNCH((resample_rows_kernel<ST>), dim3(grid), dim3(kResampleThreads), lds_bytes, stream, a);
  return true;
}

bool launch_resample_rows(const ResampleRowsArgs &a, int32_t sample_type, uint32_t lds_bytes, hipStream_t stream)
{
  switch (sample_type) {
    case AAD_HIP_SAMPLE_INT16: return launch_type<AAD_HIP_SAMPLE_INT16>(a, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT32: return launch_type<AAD_HIP_SAMPLE_FLOAT32>(a, lds_bytes, stream);
    case AAD_HIP_SAMPLE_FLOAT16: return launch_type<AAD_HIP_SAMPLE_FLOAT16>(a, lds_bytes, stream);
    default: return launch_type<AAD_HIP_SAMPLE_BFLOAT16>(a, lds_bytes, stream);
  }
}

} /* namespace aad */
