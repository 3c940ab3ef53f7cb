/* aad_window_reconstruct.hip - translation unit of the window reconstruct run's own kernel (aad_window_reconstruct.hip.h).
 *
 * window_resolve_kernel, two duties in one dispatch:
 *   resolve  one lane per (window, chain).  It reads the window and its source descriptor and writes what the host writes at plan
 *            creation for every other encode plan: the lane's StreamDesc (or ChainDesc of a segmented plan), its output base and
 *            its statistics row - by the functions of aad_windows.h, which the CPU test holds to the host builders.  The encoder
 *            launch behind it on the same stream reads those tables as it reads any plan's.
 *   tails    (runs with rows) every row element in [len_w, T) becomes zero.  A workgroup takes 256 windows: each thread works out
 *            one window's len_w, and the workgroup then zeroes, together, the rows of those that end short - none, for crops drawn
 *            inside their streams, at the price of one pass over a 1 KiB LDS array.  16-byte stores at the row's own alignment,
 *            scalar head and tail.  The encoders store frames below len_w only, so the two never write the same element. */
#include "aad_window_reconstruct.hip.h"
#include "aad_launch.h"

namespace aad {

static_assert(sizeof(AADHipStreamDesc) == 32, "the unsegmented lane table is a stream table");

typedef uint32_t u32x4_zero __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ void zero_span(T *p, uint64_t n)
{
  constexpr uint64_t kPer = 16 / sizeof(T);
  uint64_t head = ((16u - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(T);
  if (head > n) head = n;
  for (uint64_t i = threadIdx.x; i < head; i += blockDim.x) p[i] = (T)0;
  const uint64_t vectors = (n - head) / kPer;
  u32x4_zero *q = reinterpret_cast<u32x4_zero *>(p + head);
  for (uint64_t i = threadIdx.x; i < vectors; i += blockDim.x) q[i] = u32x4_zero{0, 0, 0, 0};
  for (uint64_t i = head + vectors * kPer + threadIdx.x; i < n; i += blockDim.x) p[i] = (T)0;
}

__device__ __forceinline__ void resolve_lane(const WindowResolveArgs &a, uint64_t lane)
{
  const uint32_t per = a.g.chains_per_window;
  const uint64_t w = lane / per;
  const uint32_t k = (uint32_t)(lane % per);
  const uint64_t stream = a.windows[2 * w], first_frame = a.windows[2 * w + 1];
  const uint32_t len = window_length(stream, first_frame, a.g.frames, a.num_sources, a.sources);
  const WindowLane r = window_lane(a.g, w, k, len != 0 ? a.sources[stream].pcm_offset : 0, first_frame, len);
  if (a.g.segment_blocks == 0) {
    AADHipStreamDesc d;
    d.pcm_offset = r.pcm_offset;
    d.data_offset = r.data_offset;
    d.data_size = 0; /* read by the byte ring only, which these runs never take */
    d.num_samples = r.num_frames;
    d.reserved = 0;
    static_cast<AADHipStreamDesc *>(a.table)[lane] = d;
  } else {
    ChainDesc c;
    c.pcm_offset = r.pcm_offset;
    c.data_offset = r.data_offset;
    c.first_block = r.first_block;
    c.num_frames = r.num_frames;
    c.warmup_blocks = r.warmup_blocks;
    c.header_samples = r.header_samples;
    c.writes_header = r.writes_header;
    static_cast<ChainDesc *>(a.table)[lane] = c;
  }
  a.out_base[lane] = r.out_base;
  a.stats_stream[lane] = r.stats_stream;
}

__global__ void __launch_bounds__(256) window_resolve_kernel(WindowResolveArgs a)
{
  __shared__ uint32_t lens[256];
  const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane < a.num_windows * a.g.chains_per_window) resolve_lane(a, lane);
  if (a.out == nullptr) return; /* uniform: no rows, no tails */
  for (uint64_t first = (uint64_t)blockIdx.x * 256u; first < a.num_windows; first += (uint64_t)gridDim.x * 256u) {
    const uint64_t mine = first + threadIdx.x;
    lens[threadIdx.x] = mine < a.num_windows ? window_length(a.windows[2 * mine], a.windows[2 * mine + 1], a.g.frames, a.num_sources, a.sources)
                                             : a.g.frames;
    __syncthreads();
    for (uint32_t j = 0; j < 256u; j++) {
      const uint32_t len = lens[j]; /* the same for every thread: the branch is uniform */
      if (len == a.g.frames) continue;
      for (uint32_t c = 0; c < a.channels; c++) {
        const uint64_t at = (first + j) * a.g.out_stream_stride + c * a.out_channel_stride + len, n = a.g.frames - len;
        if (a.out_float32) zero_span(static_cast<float *>(a.out) + at, n);
        else zero_span(static_cast<int16_t *>(a.out) + at, n);
      }
    }
    __syncthreads();
  }
}

void launch_window_resolve(const WindowResolveArgs &a, hipStream_t stream)
{
  const uint64_t lanes = a.num_windows * a.g.chains_per_window; /* <= UINT32_MAX: checked by the run; >= num_windows */
  AAD_LAUNCH(window_resolve_kernel, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, stream, a);
}

} /* namespace aad */
