/* aad_convolve_stats.hip - translation unit of the convolve stage's statistics kernels (AADHip_ConvolverRunStats, include/aad_hip.h
 * "reverberation"), in namespace aad::convolve_levels: a unit and a namespace of their own, so that the code objects of
 * aad_convolve.hip stay what they were and namespace aad::convolve holds that unit's kernels and no other.
 *
 * convolve_rows_stats_kernel<ST>  ST: a sample type, or kNoRows for the statistics-only run.  rows_stats_body over the unchanged
 *   convolve_tile (aad_convolve_tile.hip.h) with the statistics in the emit functor - resample_rows_stats_body's scheme
 *   (aad_resample_tile.hip.h) over a tile of 4096 outputs.
 *
 * Items as the plain kernel's, (row, tile), over the crop indices n < Le.  A thread owns up to 16 outputs of a tile (4 blocks x 4
 * accumulator registers) and keeps sum v * v (64 bits; one u * u <= 2^30 fits 32 bits before it is widened), sum |v| (<= 2^19) and
 * max |v| of them, v the int16 value of the row whatever the sample type.  The wave reduces them across its lanes, the four waves
 * meet in 96 bytes of LDS beside the 16 KB of planes, and thread 0 ends the tile with two 64-bit atomic adds and one atomic max
 * into the row's record - none where the tile is silent: the clear's zeros stand.  The thread that owns crop index 0 stores
 * `count` with a plain store.
 *
 * Barriers.  Every thread of the workgroup reaches every barrier of an item or none:
 *   - the two early exits - a window without a response, n0 >= Le - depend on the item alone, not on the thread;
 *   - a wave without a block of a short last tile (convolve_tile's mine == 0) emits nothing, yet it runs convolve_tile's staging
 *     loops and barriers, reduces its zeros and WRITES them into its slot of the scratch: thread 0 adds four slots, and a slot
 *     kept from an earlier tile would be counted twice;
 *   - the scratch of an item is read by thread 0 behind the item's last barrier.  The next item of the workgroup's item loop
 *     that writes the scratch does so behind convolve_tile, which holds at least two barriers (a response has at least one
 *     k-step, so at least one piece is staged); thread 0 reaches those only after its reads, in program order, and so no wave
 *     passes them earlier.  An item that leaves early touches neither the scratch nor a barrier. */
#include "aad_convolve_tile.hip.h"

namespace aad {
namespace convolve_levels {

using convolve::StatsArgs;

static_assert(sizeof(AADHipRowStats) == 4 * sizeof(unsigned long long), "statistics record layout");
constexpr int kNoRows = -1; /* ST of the statistics-only kernel */

template <int ST>
__device__ __forceinline__ void rows_stats_body(const StatsArgs &m)
{
  constexpr bool ROWS = ST != kNoRows;
  constexpr int OUT = ROWS ? ST : AAD_HIP_SAMPLE_INT16;
  typedef typename ResampleOut<OUT>::T T;
  const convolve::RowsArgs &a = m.r;
  __shared__ __attribute__((aligned(16))) uint32_t lds[2 * kConvolveSpan / 4];
  __shared__ unsigned long long scratch[3 * (kConvolveThreads / 64)];
  const uint32_t tid = threadIdx.x;
  const uint64_t items = a.rows * a.tiles;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t row = item / a.tiles, w = row / a.channels;
    const uint32_t n0 = (uint32_t)(item - row * a.tiles) * kConvolveTile;
    const ResampleSpan s = resample_span(m.spans, w, a.frames);
    const uint32_t response = __builtin_amdgcn_readfirstlane(a.lanes[w].response);
    const uint32_t shift = __builtin_amdgcn_readfirstlane(a.lanes[w].shift);
    const bool has_response = response < a.num_responses;
    unsigned long long *const rec = m.stats + 4 * row;
    if (n0 == 0 && tid == 0)
      rec[3] = has_response ? convolve_output_count(m.source_stats[4 * row + 3], a.source_frames, shift, s.le) : 0ull;
    if (n0 >= s.le) continue;
    const uint32_t n_end = s.le - n0 < kConvolveTile ? s.le : n0 + kConvolveTile;
    T *const out = ROWS ? static_cast<T *>(a.out) + row * a.frames : nullptr;
    if (!has_response) { /* +0 rows, the record stays zeros */
      if (ROWS)
        for (uint32_t n = n0 + tid; n < n_end; n += kConvolveThreads) out[n] = (T)0;
      continue;
    }
    const convolve::ResponseDesc d = a.responses[response];
    unsigned long long sum_sq = 0;
    uint32_t sum_abs = 0, max_abs = 0; /* sixteen outputs: at most 2^19 */
    convolve::convolve_tile(a, lds, d, row, shift, n0, n_end, [&](uint32_t n, int64_t acc) {
      if (ROWS) out[n] = convolve::element<OUT>(acc, d.q);
      const int32_t v = convolve_int16(acc, d.q);
      const uint32_t u = (uint32_t)(v < 0 ? -v : v);
      sum_sq += (unsigned long long)(u * u); /* 2^30 at the most */
      sum_abs += u;
      max_abs = u > max_abs ? u : max_abs;
    });
#pragma unroll
    for (int lanes = 32; lanes >= 1; lanes >>= 1) {
      sum_sq += __shfl_xor(sum_sq, lanes);
      sum_abs += __shfl_xor(sum_abs, lanes); /* 64 lanes: at most 2^25 */
      const uint32_t other = __shfl_xor(max_abs, lanes);
      max_abs = other > max_abs ? other : max_abs;
    }
    if ((tid & 63u) == 0) { /* a wave without a block writes its zeros */
      unsigned long long *const mine = scratch + 3 * (tid >> 6);
      mine[0] = sum_sq;
      mine[1] = sum_abs;
      mine[2] = max_abs;
    }
    __syncthreads(); /* the next tile writes the scratch behind convolve_tile's barriers, which thread 0 reaches after these reads */
    if (tid == 0) {
      unsigned long long sq = 0, ab = 0, mx = 0;
      for (uint32_t wave = 0; wave < kConvolveThreads / 64; wave++) {
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

template <int ST>
__global__ void __launch_bounds__(kConvolveThreads) convolve_rows_stats_kernel(StatsArgs m)
{
  rows_stats_body<ST>(m);
}

template <int ST>
static void launch_type(const StatsArgs &a, hipStream_t stream)
{
  AAD_LAUNCH((convolve_rows_stats_kernel<ST>), dim3(convolve::grid(a.r)), dim3(kConvolveThreads), 0, stream, a);
}

void launch_rows_stats(const StatsArgs &a, int32_t sample_type, hipStream_t stream)
{
  if (a.r.out == nullptr) return launch_type<kNoRows>(a, stream);
  switch (sample_type) {
    case AAD_HIP_SAMPLE_INT16: return launch_type<AAD_HIP_SAMPLE_INT16>(a, stream);
    case AAD_HIP_SAMPLE_FLOAT32: return launch_type<AAD_HIP_SAMPLE_FLOAT32>(a, stream);
    case AAD_HIP_SAMPLE_FLOAT16: return launch_type<AAD_HIP_SAMPLE_FLOAT16>(a, stream);
    default: return launch_type<AAD_HIP_SAMPLE_BFLOAT16>(a, stream);
  }
}

} /* namespace convolve_levels */
} /* namespace aad */
