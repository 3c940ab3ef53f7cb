/* aad_resample_tile.hip.h - the bodies of the resample stage's FIR kernels, for the two units that instantiate them:
 * aad_resample.hip (a plain resampler: the bank of a row's window whole in LDS) and aad_resample_wide.hip (a wide one: the bank
 * whole, or the rows of it a round of outputs uses).  Device code only.
 *
 * A kernel is a body - plain rows, rows with gain and spans, level statistics - over a TILE: the functor that computes acc of one
 * tile's outputs and hands each to the body's emit(n, acc).  ResampleResident is resample_tile, the only tile until the wide
 * resampler; ResampleWide (aad_resample_wide.hip) picks resample_tile or resample_tile_gathered per row.  The row writers, the
 * span clipping, STORE's zeros, the statistics reduction and `count` are the bodies' and so the same under either tile.
 *
 * resample_tile  One workgroup per (window, channel row, tile of 1024 outputs); thread tid produces outputs tile + tid + 256 j,
 *   so a wave's stores are 64 adjacent elements.  The bank of the row's window (uniform per workgroup) goes into LDS, phase p's
 *   K taps at p * stride int16 (resample_lds_stride: an odd number of words, adjacent outputs read different phases), and the
 *   span of the source row the tile reads behind it, zero where the row has no frame.  The span starts on a 4-byte boundary of
 *   the source buffer, so the row is read in whole words.  Output n = (i, p): acc = sum_k h[p][k] x[i + k], two taps per v_dot2:
 *   the coefficient pair is one word of the phase's row, the sample pair one word of the span, or - for a thread whose first
 *   sample sits at an odd element - the middle of two words, one v_alignbit; four pairs a round, their eight LDS reads issued
 *   together.  int16 x int16 into int32 is exact: sum |h| <= 65535 per phase.  Then the sample type's conversion
 *   (include/aad_hip.h "resample") and one ordinary store.
 *   A workgroup that takes a further item (grids past 2^20 workgroups) keeps its bank when the next row's is the same. */
#ifndef AAD_RESAMPLE_TILE_HIP_H
#define AAD_RESAMPLE_TILE_HIP_H

#include "aad_resample.hip.h"
#include "aad_launch.h"

namespace aad {

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

/* where a tile's span of the source row sits: element e of the span is the source row's frame jb + e, jb on a 4-byte boundary of
 * the buffer; the tile's first output reads from element front + 0, its first source frame being i0 */
struct ResampleSpanAt {
  uint32_t i0, front;
};

/* The span of the source row that outputs n0 ... n_end - 1 of bank d read, into span_words; every thread of the workgroup. */
__device__ __forceinline__ ResampleSpanAt resample_stage_span(const ResampleRowsArgs &a, const ResampleBankDesc &d,
                                                              uint32_t *span_words, uint64_t row, uint32_t shift, uint32_t n0,
                                                              uint32_t n_end)
{
  const uint32_t tid = threadIdx.x;
  const uint32_t half = d.K / 2;
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
  return ResampleSpanAt{i0, front};
}

/* acc of one output: K = 2 * half taps, the coefficient pairs at h, the sample pairs from span element e0 on */
__device__ __forceinline__ int32_t resample_dot(const uint32_t *span_words, const uint32_t *h, uint32_t e0, uint32_t half)
{
  const uint32_t *x = span_words + (e0 >> 1);
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
  return acc;
}

/* One tile of one row with a bank, for every FIR kernel: the bank into LDS unless `staged` says it is there, the span of the source
 * row behind it, then acc of the outputs n0 + tid + 256 j < n_end, each handed to emit(n, acc).  Uniform over the workgroup. */
template <class Emit>
__device__ __forceinline__ void resample_tile(const ResampleRowsArgs &a, uint32_t *bank_words, uint32_t *span_words, uint32_t &staged,
                                              uint64_t row, uint32_t bank, uint32_t shift, uint32_t n0, uint32_t n_end, Emit emit)
{
  const uint32_t tid = threadIdx.x;
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
  const ResampleSpanAt at = resample_stage_span(a, d, span_words, row, shift, n0, n_end);
  __syncthreads();
  /* (256 M) div / mod L: taken only by outputs tid + 256 j, j >= 1, which exist when T > 256 and then M < 2^23 */
  const uint32_t step = kResampleThreads * d.M, di = step / d.L, dp = step - di * d.L;
  uint32_t n = n0 + tid;
  const uint32_t nm = n * d.M;
  uint32_t i = nm / d.L, p = nm - i * d.L;
#pragma unroll 1
  for (uint32_t j = 0; j < kResamplePerThread && n < n_end; j++, n += kResampleThreads) {
    emit(n, resample_dot(span_words, bank_words + p * stride_words, at.front + (i - at.i0), half));
    i += di;
    p += dp;
    if (p >= d.L) {
      p -= d.L;
      i += 1;
    }
  }
}

/* the tile of a plain resampler: every bank fits LDS whole */
struct ResampleResident {
  template <class Emit>
  __device__ __forceinline__ void operator()(const ResampleRowsArgs &a, uint32_t *bank_words, uint32_t *span_words, uint32_t &staged,
                                             uint64_t row, uint32_t bank, uint32_t shift, uint32_t n0, uint32_t n_end, Emit emit) const
  {
    resample_tile(a, bank_words, span_words, staged, row, bank, shift, n0, n_end, emit);
  }
};

/* ---- plain rows (AADHip_ResamplerRun) ------------------------------------------------------------------------------------------ */

template <int ST, class Tile>
__device__ __forceinline__ void resample_rows_body(const ResampleRowsArgs &a, Tile tile)
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
    tile(a, bank_words, span_words, staged, row, bank, shift, n0, n_end, [&](uint32_t n, int32_t acc) { out[n] = ResampleOut<ST>::of(acc); });
  }
}

/* ---- rows with gain and spans (AADHip_ResamplerRunGain) ------------------------------------------------------------------------- */

/* the float types' row elements to and from float32: widening is exact, narrowing the one rounding of the plain kernel */
template <int ST>
struct ResampleFloat;
template <>
struct ResampleFloat<AAD_HIP_SAMPLE_FLOAT32> {
  __device__ __forceinline__ static float widen(float v) { return v; }
  __device__ __forceinline__ static float narrow(float v) { return v; }
};
template <>
struct ResampleFloat<AAD_HIP_SAMPLE_FLOAT16> {
  __device__ __forceinline__ static float widen(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
  __device__ __forceinline__ static uint16_t narrow(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
};
template <>
struct ResampleFloat<AAD_HIP_SAMPLE_BFLOAT16> {
  __device__ __forceinline__ static float widen(uint16_t v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }
  __device__ __forceinline__ static uint16_t narrow(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }
};

/* p = fl32(g * f), ADD: fl32(old + p), then the type's one rounding: two instructions, each result a register value of its own,
 * never an fma and never a product that reaches the 2-byte pack unrounded (WindowRow::gained / ::sum, aad_decode_window.hip.h) */
template <int ST, bool ADD>
__device__ __forceinline__ void resample_gain_put(typename ResampleOut<ST>::T *q, float g, float f)
{
#pragma clang fp contract(off)
  float p = g * f;
  asm("" : "+v"(p));
  if (ADD) {
    float s = ResampleFloat<ST>::widen(*q) + p;
    asm("" : "+v"(s));
    p = s;
  }
  *q = ResampleFloat<ST>::narrow(p);
}

/* the span of window w clipped to the row: Le crop indices that land at row elements o ... o + Le - 1 */
struct ResampleSpan {
  uint64_t o;
  uint32_t le;
};
__device__ __forceinline__ ResampleSpan resample_span(const uint64_t *spans, uint64_t w, uint32_t frames)
{
  ResampleSpan s = {0, frames};
  if (spans != nullptr) {
    s.o = spans[2 * w + 1];
    s.le = (uint32_t)resample_span_frames(spans[2 * w], s.o, frames); /* <= frames */
  }
  return s;
}

/* Items as the plain kernel's, (row, tile): the tile's crop indices n < Le go through the FIR and land at o + n; under STORE the
 * workgroup also writes +0 to the row elements of its tile that lie outside the span (window_fill_tile with the tile as the
 * block), so every element of a row is written exactly once, by one thread. */
template <int ST, bool ADD, class Tile>
__device__ __forceinline__ void resample_rows_gain_body(const ResampleMixArgs &m, Tile tile)
{
  typedef typename ResampleOut<ST>::T T;
  const ResampleRowsArgs &a = m.r;
  extern __shared__ __attribute__((aligned(16))) uint32_t resample_lds[];
  uint32_t *const bank_words = resample_lds;
  uint32_t *const span_words = resample_lds + a.bank_elements / 2;
  const uint32_t tid = threadIdx.x;
  const uint64_t items = a.rows * a.tiles;
  uint32_t staged = ~0u;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.tiles, w = row / a.channels;
    const uint32_t tile_index = (uint32_t)(item - row * a.tiles), n0 = tile_index * kResampleTile;
    const ResampleSpan s = resample_span(m.spans, w, a.frames);
    T *const out = static_cast<T *>(a.out) + row * a.frames;
    if (!ADD) {
      const WindowFillTile fill = window_fill_tile(tile_index, kResampleTile, 0, a.frames, s.o, s.le);
      for (int piece = 0; piece < 2; piece++)
        for (int64_t e = fill.lo[piece] + tid; e < fill.hi[piece]; e += kResampleThreads) out[e] = (T)0;
    }
    if (n0 >= s.le) continue;
    const uint32_t n_end = s.le - n0 < kResampleTile ? s.le : n0 + kResampleTile;
    T *const dst = out + s.o; /* o < T: Le > 0 */
    const float g = m.gain != nullptr ? m.gain[w] : 1.0f;
    const uint32_t bank = __builtin_amdgcn_readfirstlane(a.lanes[w].bank);
    if (bank >= a.num_banks) { /* no bank: f = +0 */
      for (uint32_t n = n0 + tid; n < n_end; n += kResampleThreads) resample_gain_put<ST, ADD>(dst + n, g, 0.0f);
      continue;
    }
    const uint32_t shift = __builtin_amdgcn_readfirstlane(a.lanes[w].shift);
    tile(a, bank_words, span_words, staged, row, bank, shift, n0, n_end,
         [&](uint32_t n, int32_t acc) { resample_gain_put<ST, ADD>(dst + n, g, (float)acc * 0x1p-29f); });
  }
}

/* ---- level statistics of the resampled rows (AADHip_ResamplerRunStats) ---------------------------------------------------------- */

static_assert(sizeof(AADHipRowStats) == 4 * sizeof(unsigned long long), "statistics record layout");
constexpr int kResampleNoRows = -1; /* ST of the statistics-only kernel */

/* Items as the plain kernel's over the crop indices n < Le.  A thread keeps sum v * v, sum |v| and max |v| of its up to four
 * outputs, v the int16 value of the row whatever the sample type; the wave reduces them across its lanes, the four waves through
 * the scratch behind the span, and thread 0 ends the tile with two 64-bit atomic adds and one atomic max into the row's record -
 * none where the tile is silent, the clear's zeros stand.  The thread that owns crop index 0 stores `count`. */
template <int ST, class Tile>
__device__ __forceinline__ void resample_rows_stats_body(const ResampleMixArgs &m, Tile tile)
{
  constexpr bool ROWS = ST != kResampleNoRows;
  typedef ResampleOut<ROWS ? ST : AAD_HIP_SAMPLE_INT16> Out;
  typedef typename Out::T T;
  const ResampleRowsArgs &a = m.r;
  extern __shared__ __attribute__((aligned(16))) uint32_t resample_lds[];
  uint32_t *const bank_words = resample_lds;
  uint32_t *const span_words = resample_lds + a.bank_elements / 2;
  unsigned long long *const scratch = reinterpret_cast<unsigned long long *>(resample_lds + m.scratch_words);
  const uint32_t tid = threadIdx.x;
  const uint64_t items = a.rows * a.tiles;
  uint32_t staged = ~0u;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.tiles, w = row / a.channels;
    const uint32_t n0 = (uint32_t)(item - row * a.tiles) * kResampleTile;
    const ResampleSpan s = resample_span(m.spans, w, a.frames);
    const uint32_t bank = __builtin_amdgcn_readfirstlane(a.lanes[w].bank);
    const uint32_t shift = __builtin_amdgcn_readfirstlane(a.lanes[w].shift);
    const bool has_bank = bank < a.num_banks;
    unsigned long long *const rec = m.stats + 4 * row;
    if (n0 == 0 && tid == 0) {
      unsigned long long count = 0;
      if (has_bank) {
        const ResampleBankDesc d = a.banks[bank];
        count = resample_output_count(m.source_stats[4 * row + 3], a.source_frames, shift, d.L, d.M, s.le);
      }
      rec[3] = count;
    }
    if (n0 >= s.le) continue;
    const uint32_t n_end = s.le - n0 < kResampleTile ? s.le : n0 + kResampleTile;
    T *const out = ROWS ? static_cast<T *>(a.out) + row * a.frames : nullptr;
    if (!has_bank) { /* +0 rows, the record stays zeros */
      if (ROWS)
        for (uint32_t n = n0 + tid; n < n_end; n += kResampleThreads) out[n] = (T)0;
      continue;
    }
    unsigned long long sum_sq = 0;
    uint32_t sum_abs = 0, max_abs = 0; /* four outputs: at most 2^17 */
    tile(a, bank_words, span_words, staged, row, bank, shift, n0, n_end, [&](uint32_t n, int32_t acc) {
      if (ROWS) out[n] = Out::of(acc);
      const int32_t v = ResampleOut<AAD_HIP_SAMPLE_INT16>::of(acc);
      const uint32_t u = (uint32_t)(v < 0 ? -v : v);
      sum_sq += (unsigned long long)(u * u); /* 2^30 at the most */
      sum_abs += u;
      max_abs = u > max_abs ? u : max_abs;
    });
#pragma unroll
    for (int lanes = 32; lanes >= 1; lanes >>= 1) {
      sum_sq += __shfl_xor(sum_sq, lanes);
      sum_abs += __shfl_xor(sum_abs, lanes); /* 64 lanes: at most 2^23 */
      const uint32_t other = __shfl_xor(max_abs, lanes);
      max_abs = other > max_abs ? other : max_abs;
    }
    if ((tid & 63u) == 0) {
      unsigned long long *const mine = scratch + 3 * (tid >> 6);
      mine[0] = sum_sq;
      mine[1] = sum_abs;
      mine[2] = max_abs;
    }
    __syncthreads(); /* the next tile writes the scratch behind the tile's barriers, which thread 0 reaches after these reads */
    if (tid == 0) {
      unsigned long long sq = 0, ab = 0, mx = 0;
      for (uint32_t wave = 0; wave < kResampleThreads / 64; wave++) {
        sq += scratch[3 * wave];
        ab += scratch[3 * wave + 1];
        mx = scratch[3 * wave + 2] > mx ? scratch[3 * wave + 2] : mx;
      }
      if (mx != 0) {
        atomicAdd(rec, sq);
        atomicAdd(rec + 1, ab);
        atomicMax(rec + 2, mx);
      }
    }
  }
}

/* the grid of every FIR launch: one workgroup per item up to 2^20, the kernels' item loop takes the rest */
inline uint32_t resample_grid(const ResampleRowsArgs &a)
{
  const uint64_t items = a.rows * a.tiles;
  return items < (1u << 20) ? (uint32_t)items : (1u << 20);
}

} /* namespace aad */

#endif /* AAD_RESAMPLE_TILE_HIP_H */
