/*
 * aad_hip_engine.hip - host side of the batched C-ABI declared in include/aad_hip.h: contexts, plans (uploaded stream tables), kernel
 * launches and the host-memory convenience calls.  Device code lives in aad_encode.hip.h / aad_decode.hip.h (shared parts:
 * aad_device.hip.h) and, for the split, sector-tiled and window decoders and the planar-input and planar reconstruct encoders, in
 * units of their own (aad_decode_split.hip, aad_decode_tiled.hip, aad_decode_window.hip, aad_encode_units.hip - one object per input
 * type and REC; the window reconstruct run's resolve kernel: aad_window_reconstruct.hip).  Every kind of encode plan is made by
 * encode_plan_create and run by encode_plan_run over one description of a run (aad::EncodeRun, aad_encode_launch.hip.h), which the
 * host-memory paths build directly.  The FIR stages behind a window decode (AADHip_Resampler*, AADHip_Convolver*) have a host unit
 * of their own, aad_fir_stage.hip; the context and the helpers that both units use are aad_hip_context.hip.h's.  gfx950 only; no
 * CPU code path - every entry point that needs the GPU fails with AAD_APIRESULT_NG when HIP does.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/aad_hip.h"
#include "aad_compare.hip.h"
#include "aad_decode.hip.h"
#include "aad_decode_window.hip.h"
#include "aad_encode.hip.h"
#include "aad_encode_launch.hip.h"
#include "aad_format.h"
#include "aad_hip_context.hip.h" /* and aad_launch.h, aad_launch_policy.h */
#include "aad_hip_internal.h"
#include "aad_tiles.h"
#include "aad_window_reconstruct.hip.h"

namespace aad {
thread_local LaunchSignal tl_launch_signal = {nullptr, nullptr}; /* aad_launch.h */
}

static_assert(sizeof(AADHipStreamDesc) == sizeof(aad::StreamDesc), "stream table layout");
static_assert(sizeof(AADHipLaneState) == sizeof(aad::LaneStateRecord), "lane state layout");
static_assert(sizeof(AADHipErrorStats) == sizeof(aad::ErrorStatsRecord), "error stats layout");

/* A few helper threads that only ever memcpy: the staging copies between the caller's pageable buffers
 * and the pinned blocks are the slowest stage of the host-memory path (one core moves ~10 GB/s, PCIe
 * ~50 GB/s), so chunks of a megabyte and more are filled and drained by up to four threads, each on a
 * contiguous range of streams.  Started at a context's first such chunk, joined in ContextDestroy; no
 * HIP call is ever made from them. */
struct StagingPool {
  std::vector<std::thread> threads;
  std::mutex lock;
  std::condition_variable work, done;
  std::function<void(unsigned)> job;
  unsigned generation = 0, pending = 0;
  bool stop = false;
};

/* which of the three ...PlanRun entry points runs a plan: they take different pointers */
enum class EncodePlanKind {
  Frames,      /* AADHip_EncodePlanCreate, AADHip_SegmentedEncodePlanCreate -> AADHip_EncodePlanRun */
  Rows,        /* AADHip_PlanarEncodePlanCreate -> AADHip_PlanarEncodePlanRun */
  Reconstruct, /* AADHip_PlanarReconstructPlanCreate -> AADHip_PlanarReconstructPlanRun */
  Windows      /* AADHip_WindowReconstructPlanCreate -> AADHip_WindowReconstructPlanRun */
};

/* what a window reconstruct plan holds besides its run: the lanes are written on the device, per run, from the window table */
struct WindowPlanPart {
  AADHipSegmentation seg;    /* segment_blocks == 0: unsegmented */
  AADEncodeParameter parameter;
  AADHipStreamDesc *d_sources;
  uint32_t num_sources;
  uint8_t *d_lanes;          /* the lane tables of the largest run so far: table | out_base | stats_stream, grow-only */
  uint64_t lanes_capacity;   /* in bytes */
};

struct AADHipEncodePlan { /* every field is set by encode_plan_create */
  AADHipContext *ctx;
  EncodePlanKind kind;
  aad::EncodeRun run;   /* all of a run but the caller's pointers (args.pcm / data / state / state_out, rows.out) */
  void *d_table;        /* run.args.streams, or run.args.chains of a segmented plan */
  uint64_t *d_out_base; /* Reconstruct: run.rows.base, else null */
  uint32_t *d_stats_stream; /* Reconstruct, segmented: run.stats_stream, else null */
  uint64_t stats_records;   /* Reconstruct: streams * channels, the records of a statistics table */
  WindowPlanPart *windows;  /* Windows (then `run` has no table, lane count, output or pointer: they come with each run), else null */
};

struct AADHipDecodePlan {
  AADHipContext *ctx;
  aad::DecodeArgs args;
  aad::StreamDesc *d_streams;
  uint64_t *d_prefix;
};

/* AADHip_WindowDecodePlanCreate (Same): `args` is the format and the table (decode_plan_init); AADHip_MixedWindowDecodePlanCreate,
 * AADHip_ChannelMixWindowDecodePlanCreate: it holds the table, the channel count (ChannelMix: the OUTPUT's) and header_bytes alone,
 * and the formats are d_formats'.  The windows come with each run */
struct AADHipWindowDecodePlan {
  AADHipContext *ctx = nullptr;
  aad::WindowKind kind = aad::WindowKind::Same;
  aad::DecodeArgs args = {};
  aad::StreamDesc *d_streams = nullptr;
  void *d_formats = nullptr; /* Mixed: aad::StreamFormat, ChannelMix: aad::ChannelStreamFormat, one record per stream; Same: null */
  aad::WindowVariants variants = {}; /* the launches of a run (plan_window_run); Same: the one variant of the header */
};

struct AADHipReconstructPlan {
  AADHipContext *ctx;
  AADHipEncodePlan *encode;
  AADHipDecodePlan *decode;
  aad::CompareArgs args; /* streams -> the decode plan's table */
  uint64_t *d_segment_prefix;
  aad::ErrorPartial *d_partials;
};

namespace {

/* arithmetic-progression stream tables get the table-free kernel path (aad::UniformLayout) */
aad::UniformLayout detect_uniform(uint32_t n, const AADHipStreamDesc *t)
{
  aad::UniformLayout u;
  memset(&u, 0, sizeof(u));
  if (n == 0) return u;
  const uint64_t ps = n > 1 ? t[1].pcm_offset - t[0].pcm_offset : 0, ds = n > 1 ? t[1].data_offset - t[0].data_offset : 0;
  for (uint32_t i = 0; i < n; i++) {
    if (t[i].num_samples != t[0].num_samples || t[i].data_size != t[0].data_size) return u;
    if (t[i].pcm_offset != t[0].pcm_offset + (uint64_t)i * ps || t[i].data_offset != t[0].data_offset + (uint64_t)i * ds) return u;
  }
  u.pcm_base = t[0].pcm_offset;
  u.pcm_stride = ps;
  u.data_base = t[0].data_offset;
  u.data_stride = ds;
  u.data_size = t[0].data_size;
  u.num_samples = t[0].num_samples;
  u.enabled = 1;
  return u;
}

bool staging_reserve(AADHipContext *ctx, Staging &st, size_t bytes)
{
  if (bytes <= st.cap) return true;
  if (st.host) (void)hipHostFree(st.host);
  if (st.dev) (void)hipFree(st.dev);
  st.host = st.dev = nullptr;
  st.cap = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  if (!hip_ok(ctx, hipHostMalloc(&st.host, want, hipHostMallocDefault), "hipHostMalloc")) return false;
  if (!hip_ok(ctx, hipMalloc(&st.dev, want), "hipMalloc staging")) return false;
  st.cap = want;
  return true;
}

void staging_release(Staging &st)
{
  if (st.host) (void)hipHostFree(st.host);
  if (st.dev) (void)hipFree(st.dev);
  st = Staging();
}

/* ---- dispatch: from a plan (aad_launch_policy.h) to a template instantiation ---------------------------------------------- */
/* the encoders: aad_encode_launch.hip.h */

/* decode_blocks_kernel by channels and M/S; the dense stereo 4- / 2-bit kernels in their streamed-store form when the plan says so */
template <int BITS, bool QUAD>
void launch_decode_mapped(const aad::DecodeArgs &a, const aad::DecodeLaunch &p, hipStream_t stream)
{
  const dim3 grid(p.grid), block(p.workgroup);
  if (a.channels == 1)
    AAD_LAUNCH((aad::decode_blocks_kernel<BITS, 1, false, QUAD>), grid, block, p.lds, stream, a);
  else if (a.channels == 2 && a.mid_side) {
    if constexpr (!QUAD && BITS != 3) {
      if (p.stream_stores) {
        AAD_LAUNCH((aad::decode_blocks_kernel<BITS, 2, true, false, true>), grid, block, p.lds, stream, a);
        return;
      }
    }
    AAD_LAUNCH((aad::decode_blocks_kernel<BITS, 2, true, QUAD>), grid, block, p.lds, stream, a);
  } else if (a.channels == 2) {
    if constexpr (!QUAD && BITS != 3) {
      if (p.stream_stores) {
        AAD_LAUNCH((aad::decode_blocks_kernel<BITS, 2, false, false, true>), grid, block, p.lds, stream, a);
        return;
      }
    }
    AAD_LAUNCH((aad::decode_blocks_kernel<BITS, 2, false, QUAD>), grid, block, p.lds, stream, a);
  }
  else if constexpr (!QUAD)
    AAD_LAUNCH((aad::decode_blocks_kernel<BITS, 0, false, false>), grid, block, p.lds, stream, a);
}

template <int BITS>
void launch_decode(const aad::DecodeArgs &a, const aad::DecodeLaunch &p, int32_t *residual, hipStream_t stream)
{
  switch (p.kernel) {
    case aad::DecodeKernel::SplitLds:
    case aad::DecodeKernel::SplitScratch: aad::launch_decode_split(a, p, residual, stream); break;
    case aad::DecodeKernel::Tiled: aad::launch_decode_tiled(a, p, stream); break;
    case aad::DecodeKernel::QuadFused: launch_decode_mapped<BITS, true>(a, p, stream); break;
    case aad::DecodeKernel::Dense: launch_decode_mapped<BITS, false>(a, p, stream); break;
  }
}
} /* namespace */

/* the window decoders: launch_window_unit (aad_launch.h), from (kind, mode, sample type) to the object that holds the kernels */
namespace aad {
template <WindowKind KIND, WindowMode MODE>
void launch_window_rows(const WindowUnitRun &r, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  if constexpr (MODE != WindowMode::PlacedStats)
    if (window_half_type(sample_type)) return launch_window_object<KIND, MODE, true>(r, p, sample_type, stream);
  launch_window_object<KIND, MODE, false>(r, p, sample_type, stream);
}
template <WindowKind KIND>
void launch_window_mode(WindowMode mode, const WindowUnitRun &r, const WindowLaunch &p, int32_t sample_type, hipStream_t stream)
{
  switch (mode) {
  case WindowMode::Rows: return launch_window_rows<KIND, WindowMode::Rows>(r, p, sample_type, stream);
  case WindowMode::Stats: return launch_window_rows<KIND, WindowMode::Stats>(r, p, sample_type, stream);
  case WindowMode::Gain: return launch_window_rows<KIND, WindowMode::Gain>(r, p, sample_type, stream);
  case WindowMode::Placed: return launch_window_rows<KIND, WindowMode::Placed>(r, p, sample_type, stream);
  case WindowMode::PlacedStats: return launch_window_rows<KIND, WindowMode::PlacedStats>(r, p, sample_type, stream);
  }
}
void launch_window_unit(WindowKind kind, WindowMode mode, const WindowUnitRun &r, const WindowLaunch &p, int32_t sample_type,
                        hipStream_t stream)
{
  switch (kind) {
  case WindowKind::Same: return launch_window_mode<WindowKind::Same>(mode, r, p, sample_type, stream);
  case WindowKind::Mixed: return launch_window_mode<WindowKind::Mixed>(mode, r, p, sample_type, stream);
  case WindowKind::ChannelMix: return launch_window_mode<WindowKind::ChannelMix>(mode, r, p, sample_type, stream);
  }
}
} /* namespace aad */

/* ---- plan construction without any device work ------------------------------------------------
 * Validation + launch arguments.  AADHip_*PlanCreate adds the table upload; the host-memory
 * calls put the tables into the block that carries the payload instead. */
namespace {

/* lead_frames: context frames at the head of every stream (EncodeArgs::lead_frames) - 0, or one block */
AADApiResult encode_plan_init(const struct AADEncodeParameter *parameter, uint32_t num_streams,
                              const struct AADHipStreamDesc *streams, aad::EncodeArgs *args, uint32_t lead_frames = 0,
                              bool streams_checked = false)
{
  AADHeaderInfo h;
  if (AADFormat_ParameterToHeader(parameter, 1, AAD_HIP_MAX_NUM_CHANNELS, &h) != AAD_APIRESULT_OK)
    return AAD_APIRESULT_INVALID_FORMAT;
  /* what AADEncoder_EncodeHeader would reject (bits == 1, zero rate, M/S on mono, ...) */
  if (!AADFormat_HeaderFieldsValid(&h, AAD_HIP_MAX_NUM_CHANNELS)) return AAD_APIRESULT_INVALID_FORMAT;
  if (h.ch_process_method == AAD_CH_PROCESS_METHOD_MS && h.num_channels != 2) return AAD_APIRESULT_INVALID_FORMAT;
  for (uint32_t i = 0; !streams_checked && i < num_streams; i++) {
    if (streams[i].num_samples <= lead_frames) return AAD_APIRESULT_INVALID_FORMAT; /* src/aad_encoder.c:157-159 */
    h.num_samples = streams[i].num_samples - lead_frames;
    if (streams[i].data_size < AADFormat_EncodedSize(&h)) return AAD_APIRESULT_INSUFFICIENT_BUFFER;
  }
  memset(args, 0, sizeof(*args));
  args->num_streams = num_streams;
  args->channels = h.num_channels;
  args->block_size = h.block_size;
  args->samples_per_block = h.num_samples_per_block;
  args->mid_side = h.ch_process_method == AAD_CH_PROCESS_METHOD_MS;
  args->trials = parameter->num_encode_trials;
  args->lead_frames = lead_frames;
  args->uni = detect_uniform(num_streams, streams);
  /* the rows' byte rings store whole 64-byte sectors of an image at their own addresses: images on 64-byte boundaries */
  args->ring_ok = 1;
  for (uint32_t i = 0; i < num_streams; i++)
    if (streams[i].data_offset % 64u != 0) {
      args->ring_ok = 0;
      break;
    }
  h.num_samples = 0;
  AADFormat_PutHeader(&h, args->header_template);
  args->bits = h.bits_per_sample;
  return AAD_APIRESULT_OK;
}

/* prefix: num_streams + 1 entries, the exclusive prefix sum of blocks per stream */
/* known_blocks: per-stream block counts of streams that an earlier call of this function has already
 * validated (the tiles of the host-memory path) - the checks and their divisions are skipped */
AADApiResult decode_plan_init(const struct AADHeaderInfo *format, int32_t has_file_header, uint32_t num_streams,
                              const struct AADHipStreamDesc *streams, uint64_t *prefix, aad::DecodeArgs *args,
                              const uint64_t *known_blocks = nullptr)
{
  AADHeaderInfo h = *format;
  h.num_samples = 1; /* per-stream counts come from the table */
  if (!AADFormat_HeaderAcceptedByDecoder(&h, AAD_HIP_MAX_NUM_CHANNELS)) return AAD_APIRESULT_INVALID_FORMAT;
  if (h.ch_process_method == AAD_CH_PROCESS_METHOD_MS && h.num_channels != 2) return AAD_APIRESULT_INVALID_FORMAT;
  uint64_t blocks = 0;
  const uint32_t head = has_file_header ? AAD_HEADER_SIZE : 0;
  for (uint32_t i = 0; known_blocks != nullptr && i < num_streams; i++) {
    prefix[i] = blocks;
    blocks += known_blocks[i];
  }
  for (uint32_t i = 0; known_blocks == nullptr && i < num_streams; i++) {
    prefix[i] = blocks;
    /* per-block loop counters on the device are 32-bit: a header that claims a block of 2^31
     * samples and more (nothing in the reference's checks forbids it) is refused here */
    if (!AADFormat_DecodeWorkBounded(&h, streams[i].num_samples)) return AAD_APIRESULT_INVALID_FORMAT;
    /* the reference walks blocks while samples remain AND bytes remain (src/aad_decoder.c:514) */
    const uint64_t by_samples = ((uint64_t)streams[i].num_samples + h.num_samples_per_block - 1) / h.num_samples_per_block;
    const uint64_t payload = streams[i].data_size > head ? streams[i].data_size - head : 0;
    const uint64_t by_bytes = (payload + h.block_size - 1) / h.block_size;
    const uint64_t nblk = by_samples < by_bytes ? by_samples : by_bytes;
    /* a present block shorter than its header is the reference's INSUFFICIENT_DATA (src/aad_decoder.c:347-349) */
    if (nblk > 0) {
      const uint64_t last_bytes = payload - (nblk - 1) * h.block_size;
      if (last_bytes < (uint64_t)AAD_BLOCK_HEADER_BYTES_PER_CH * h.num_channels) return AAD_APIRESULT_INSUFFICIENT_DATA;
    }
    blocks += nblk;
  }
  prefix[num_streams] = blocks;
  memset(args, 0, sizeof(*args));
  args->total_blocks = blocks;
  args->num_streams = num_streams;
  args->channels = h.num_channels;
  args->block_size = h.block_size;
  args->samples_per_block = h.num_samples_per_block;
  args->header_bytes = head;
  args->uni = detect_uniform(num_streams, streams);
  if (args->uni.enabled) {
    args->uni.blocks_per_stream = (uint32_t)(num_streams ? prefix[1] - prefix[0] : 0);
    if (args->uni.blocks_per_stream == 0 || blocks >= 0xFFFFFFFFull) args->uni.enabled = 0;
  }
  args->mid_side = h.ch_process_method == AAD_CH_PROCESS_METHOD_MS;
  args->bits = h.bits_per_sample;
  /* the sector-tiled dense decoder moves PCM in 16-byte pieces: every stream's PCM must start on a piece boundary */
  args->pcm_aligned16 = 1;
  for (uint32_t i = 0; i < num_streams; i++)
    if ((streams[i].pcm_offset * 2u) % 16u != 0) {
      args->pcm_aligned16 = 0;
      break;
    }
  /* ... and its 3-bit rows want every block's code bytes at the same offset inside a granule (64 bytes mono, 128 stereo): all
   * images start at the same offset inside one, and so does every block of an image */
  {
    const uint32_t granule = h.num_channels == 1 ? 64u : 128u;
    args->code_phase_uniform = (h.block_size % granule == 0) ? 1 : 2; /* 2: one-block streams only (checked at launch) */
    for (uint32_t i = 1; i < num_streams; i++)
      if ((streams[i].data_offset - streams[0].data_offset) % granule != 0) {
        args->code_phase_uniform = 0;
        break;
      }
  }
  /* Dense stereo 4-/2-bit decode opens every block with a 16-frame chunk, so its stores are whole
   * 64-byte granules exactly when every block's first frame is 64-byte aligned: a uniform layout
   * whose stream pitch and block length (in PCM bytes) are multiples of 64.  Only then are they
   * issued non-temporal (the base pointer is checked at run time). */
  args->stream_stores = args->uni.enabled && h.num_channels == 2 && h.bits_per_sample != 3 &&
                        (args->uni.pcm_base * 2) % 64 == 0 && (args->uni.pcm_stride * 2) % 64 == 0 &&
                        ((uint64_t)h.num_samples_per_block * 4) % 64 == 0;
  return AAD_APIRESULT_OK;
}

/* launch with fully populated arguments (device pointers set) on the context's stream */
/* AADHip_ContextSignalNextRun: the pending events, taken by the plan run that starts now ... */
aad::LaunchSignal take_signal(AADHipContext *ctx)
{
  const aad::LaunchSignal s = ctx->signal_next;
  ctx->signal_next = aad::LaunchSignal{nullptr, nullptr};
  return s;
}
/* ... and settled when it ends: a run that launched its kernel has handed the events to it (aad_launch.h); one that launched
 * nothing (an empty plan) records them behind whatever the stream holds; a failed run leaves them unrecorded - but for the
 * start event of a statistics run whose clear itself failed to enqueue (clear_window_stats: the event goes in front of the clear) */
AADApiResult finish_signal(AADHipContext *ctx, const aad::LaunchSignal &signal, AADApiResult rc)
{
  const bool taken = aad::tl_launch_signal.start == nullptr && aad::tl_launch_signal.stop == nullptr;
  aad::tl_launch_signal = aad::LaunchSignal{nullptr, nullptr};
  if (taken || rc != AAD_APIRESULT_OK) return rc;
  if (signal.start != nullptr && !hip_ok(ctx, hipEventRecord(signal.start, ctx->stream), "hipEventRecord")) return AAD_APIRESULT_NG;
  if (signal.stop != nullptr && !hip_ok(ctx, hipEventRecord(signal.stop, ctx->stream), "hipEventRecord")) return AAD_APIRESULT_NG;
  return rc;
}

/* grow-only device scratch of a context (dual trial search, split decoder); the old buffer may still be in use by queued work */
template <typename T>
bool scratch_reserve(AADHipContext *ctx, T **buf, uint64_t *capacity, uint64_t bytes, const char *what)
{
  if (*capacity >= bytes) return true;
  if (*buf) {
    if (!hip_ok(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) return false;
    (void)hipFree(*buf);
    *buf = nullptr;
    *capacity = 0;
  }
  if (!hip_ok(ctx, hipMalloc((void **)buf, bytes), what)) return false;
  *capacity = bytes;
  return true;
}

/* launch one encode run (aad_encode_launch.hip.h EncodeRun) with fully populated arguments on the context's stream */
AADApiResult run_encode(AADHipContext *ctx, const aad::EncodeRun &run)
{
  if (run.args.num_streams == 0) return AAD_APIRESULT_OK;
  if (run.args.bits < 2 || run.args.bits > 4) return AAD_APIRESULT_INVALID_FORMAT;
  aad::EncodeRun r = run;
  aad::EncodeArgs &a = r.args;
  if ((reinterpret_cast<uintptr_t>(a.data) & 63u) != 0) a.ring_ok = 0;
  const aad::EncodeBatch batch{a.bits, a.channels, a.num_streams, a.trials, a.block_size, a.ring_ok != 0};
  const aad::EncodeLaunch p = r.rec != aad::kRecNone ? aad::plan_reconstruct_encode(ctx->device_info, ctx->knobs, batch)
                                                     : aad::plan_encode(ctx->device_info, ctx->knobs, batch);
  a.trial_scratch = nullptr;
  a.trial_slot_bytes = p.trial_slot_bytes;
  a.simd_role = p.simd_role;
  if (p.trial_scratch_bytes != 0) {
    if (!scratch_reserve(ctx, &ctx->d_trial, &ctx->trial_capacity, p.trial_scratch_bytes, "hipMalloc trial scratch")) return AAD_APIRESULT_NG;
    a.trial_scratch = ctx->d_trial;
  }
  auto by_layout = [&](auto rec) {
    constexpr int REC = decltype(rec)::value;
    switch (r.in) {
      case aad::kInPlanarF32: aad::launch_encode_run<aad::kInPlanarF32, REC>(r, p, ctx->stream); break;
      case aad::kInPlanarI16: aad::launch_encode_run<aad::kInPlanarI16, REC>(r, p, ctx->stream); break;
      case aad::kInInterleaved: aad::launch_encode_run<aad::kInInterleaved, REC>(r, p, ctx->stream); break;
    }
  };
  switch (r.rec) {
    case aad::kRecStatsOnly: by_layout(std::integral_constant<int, aad::kRecStatsOnly>{}); break;
    case aad::kRecF32Stats: by_layout(std::integral_constant<int, aad::kRecF32Stats>{}); break;
    case aad::kRecI16Stats: by_layout(std::integral_constant<int, aad::kRecI16Stats>{}); break;
    case aad::kRecF32: by_layout(std::integral_constant<int, aad::kRecF32>{}); break;
    case aad::kRecI16: by_layout(std::integral_constant<int, aad::kRecI16>{}); break;
    case aad::kRecNone: by_layout(std::integral_constant<int, aad::kRecNone>{}); break;
  }
  return hip_ok(ctx, hipGetLastError(), "encode launch") ? AAD_APIRESULT_OK : AAD_APIRESULT_NG;
}

/* The table of a run becomes a chain table of `count` chains (aad_segments.h): chains are the kernel's streams, none of them
 * uniform, and the byte ring, which writes an image from its start (aad_encode.hip.h, SEG), is off. */
void use_chain_table(aad::EncodeRun *run, const aad::ChainDesc *chains, uint32_t count)
{
  run->chain_table = true;
  run->args.chains = chains;
  run->args.num_streams = count;
  run->args.ring_ok = 0;
  run->args.uni.enabled = 0;
}

/* what the two planar ...PlanCreate entry points ask of their layout and segmentation */
bool planar_fields_ok(const struct AADHipPlanarLayout *layout, const struct AADHipSegmentation *segmentation)
{
  if ((layout->sample_type != AAD_HIP_SAMPLE_INT16 && layout->sample_type != AAD_HIP_SAMPLE_FLOAT32) || layout->reserved != 0) return false;
  return segmentation == nullptr || segmentation->segment_blocks != 0;
}

/* Every kind of encode plan.  layout: the input is rows (AADHip_PlanarEncodePlanCreate), null: interleaved frames; output: the plan
 * also writes the decoded rows (AADHip_PlanarReconstructPlanCreate; layout non-null); segmentation: the streams are cut into
 * chains (segment_blocks != 0), null: one lane per stream.  The callers have checked their own arguments. */
AADApiResult encode_plan_create(AADHipContext *ctx, const struct AADEncodeParameter *parameter, const struct AADHipPlanarLayout *layout,
                                const struct AADHipPlanarOutput *output, const struct AADHipSegmentation *segmentation,
                                uint32_t num_streams, const struct AADHipStreamDesc *streams, struct AADHipEncodePlan **plan)
{
  aad::EncodeRun run;
  const AADApiResult rc = encode_plan_init(parameter, num_streams, streams, &run.args);
  if (rc != AAD_APIRESULT_OK) return rc;
  const aad::EncodeArgs &args = run.args;
  const char *what = layout != nullptr ? "planar encode plan" : "segmented encode plan";
  /* every row of every stream lies inside [0, 2^64) elements and bytes: the last element a stream reads is
   * pcm_offset + (C - 1) channel_stride + num_samples - 1 */
  const uint64_t elem = layout != nullptr && layout->sample_type == AAD_HIP_SAMPLE_FLOAT32 ? 4u : 2u;
  for (uint32_t i = 0; layout != nullptr && i < num_streams; i++) {
    if (args.channels > 1 && layout->channel_stride < streams[i].num_samples) {
      snprintf(ctx->last_error, sizeof(ctx->last_error), "planar encode plan: channel_stride %llu < num_samples %u of stream %u",
               (unsigned long long)layout->channel_stride, streams[i].num_samples, i);
      return AAD_APIRESULT_INVALID_ARGUMENT;
    }
    uint64_t span = 0, end = 0, bytes = 0;
    if (__builtin_mul_overflow((uint64_t)(args.channels - 1), layout->channel_stride, &span) ||
        __builtin_add_overflow(span, (uint64_t)streams[i].num_samples, &span) ||
        __builtin_add_overflow(streams[i].pcm_offset, span, &end) || __builtin_mul_overflow(end, elem, &bytes)) {
      snprintf(ctx->last_error, sizeof(ctx->last_error), "planar encode plan: the rows of stream %u overflow 64-bit offsets", i);
      return AAD_APIRESULT_INVALID_ARGUMENT;
    }
  }
  std::vector<aad::ChainDesc> chains;
  if (segmentation != nullptr &&
      !aad::build_segment_chains(streams, num_streams, args.channels, args.samples_per_block, args.block_size,
                                 segmentation->segment_blocks, segmentation->warmup_blocks, &chains, layout != nullptr)) {
    snprintf(ctx->last_error, sizeof(ctx->last_error), "%s: more than %u chains", what, (unsigned)UINT32_MAX);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  if (output != nullptr && !aad::planar_output_ok(args.channels, num_streams, streams, output)) {
    snprintf(ctx->last_error, sizeof(ctx->last_error),
             "planar reconstruct plan: output rows refused (sample type, reserved, a stride below the rows, or past 64-bit offsets)");
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  AADHipEncodePlan *p = new (std::nothrow) AADHipEncodePlan();
  if (p == nullptr) return AAD_APIRESULT_NG;
  p->ctx = ctx;
  p->kind = output != nullptr ? EncodePlanKind::Reconstruct : (layout != nullptr ? EncodePlanKind::Rows : EncodePlanKind::Frames);
  p->d_table = nullptr;
  p->d_out_base = nullptr;
  p->d_stats_stream = nullptr;
  p->windows = nullptr;
  p->stats_records = (uint64_t)num_streams * args.channels;
  DeviceGuard guard(ctx);
  bool ok = guard.ok;
  if (ok && segmentation != nullptr) {
    aad::ChainDesc *d_chains = nullptr;
    ok = upload(ctx, &d_chains, chains.data(), chains.size());
    p->d_table = d_chains;
    use_chain_table(&run, d_chains, (uint32_t)chains.size());
  } else if (ok) {
    aad::StreamDesc *d_streams = nullptr;
    ok = upload(ctx, &d_streams, reinterpret_cast<const aad::StreamDesc *>(streams), num_streams);
    p->d_table = d_streams;
    run.args.streams = d_streams;
  }
  if (ok && output != nullptr) {
    const std::vector<uint64_t> base =
        aad::reconstruct_output_bases(num_streams, output->stream_stride, segmentation != nullptr ? &chains : nullptr, args.samples_per_block);
    ok = upload(ctx, &p->d_out_base, base.data(), base.size());
    run.rec = aad::rec_output(output->sample_type);
    run.rows = aad::RecRows{nullptr, p->d_out_base, output->channel_stride};
  }
  if (ok && output != nullptr && segmentation != nullptr) { /* a statistics run's chains add into their stream's records */
    const std::vector<uint32_t> of = aad::chain_streams(chains);
    ok = upload(ctx, &p->d_stats_stream, of.data(), of.size());
    run.stats_stream = p->d_stats_stream;
  }
  if (!ok) {
    if (p->d_table) (void)hipFree(p->d_table);
    if (p->d_out_base) (void)hipFree(p->d_out_base);
    if (p->d_stats_stream) (void)hipFree(p->d_stats_stream);
    delete p;
    return AAD_APIRESULT_NG;
  }
  if (layout != nullptr) {
    run.in = aad::planar_layout(layout->sample_type, args.channels);
    run.channel_stride = layout->channel_stride;
  }
  p->run = run;
  *plan = p;
  return AAD_APIRESULT_OK;
}

/* Run a plan for the entry point that takes plans of `kind`.  samples: interleaved int16 frames (Frames), or rows that the kernels
 * read as the plan's sample type; out: the decoded rows, Reconstruct only.  with_stats (AADHip_PlanarReconstructPlanRunStats): the
 * run also writes the statistics table `stats`, and `out` may be null. */
AADApiResult encode_plan_run(AADHipEncodePlan *plan, EncodePlanKind kind, const void *samples, uint8_t *device_data, void *out,
                             struct AADHipLaneState *device_state, bool with_stats = false, struct AADHipRowStats *stats = nullptr)
{
  if (plan == nullptr || samples == nullptr || device_data == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  AADHipContext *ctx = plan->ctx;
  const aad::LaunchSignal signal = take_signal(ctx);
  DeviceGuard guard(ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  if (plan->kind != kind) return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT); /* frames, rows, rows in and out: each its own ...PlanRun */
  if (plan->run.chain_table && device_state != nullptr) return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  if (kind == EncodePlanKind::Reconstruct && out == samples) return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  if (plan->run.args.num_streams == 0) return finish_signal(ctx, signal, AAD_APIRESULT_OK);
  if (kind == EncodePlanKind::Reconstruct && out == nullptr && !with_stats) return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  if (with_stats && (stats == nullptr || (reinterpret_cast<uintptr_t>(stats) & 7u) != 0))
    return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  aad::EncodeRun r = plan->run;
  r.args.pcm = static_cast<const int16_t *>(samples);
  r.args.data = device_data;
  r.args.state = reinterpret_cast<const aad::LaneStateRecord *>(device_state);
  r.args.state_out = reinterpret_cast<aad::LaneStateRecord *>(device_state);
  r.rows.out = out;
  if (with_stats) {
    r.rec = aad::rec_with_stats(r.rec, out != nullptr);
    r.stats = stats;
  }
  if (with_stats && r.chain_table) {
    /* several chains add into a row's record: the table is cleared first, so the run is two device operations - the start event
     * in front of the clear, the stop event on the kernel */
    if (signal.start != nullptr && !hip_ok(ctx, hipEventRecord(signal.start, ctx->stream), "hipEventRecord")) return AAD_APIRESULT_NG;
    if (!hip_ok(ctx, hipMemsetAsync(stats, 0, plan->stats_records * sizeof(struct AADHipRowStats), ctx->stream), "hipMemsetAsync"))
      return AAD_APIRESULT_NG;
    const aad::LaunchSignal stop_only = {nullptr, signal.stop};
    aad::tl_launch_signal = stop_only;
    return finish_signal(ctx, stop_only, run_encode(ctx, r));
  }
  aad::tl_launch_signal = signal; /* the run's one kernel takes it (aad_launch.h) */
  return finish_signal(ctx, signal, run_encode(ctx, r));
}

AADApiResult run_decode(AADHipContext *ctx, const aad::DecodeArgs &a)
{
  if (a.total_blocks == 0) return AAD_APIRESULT_OK;
  if (a.bits < 2 || a.bits > 4) return AAD_APIRESULT_INVALID_FORMAT;
  const aad::DecodeLaunch p = aad::plan_decode(
      ctx->device_info, ctx->knobs,
      aad::DecodeBatch{a.total_blocks, a.num_streams, a.channels, a.bits, a.samples_per_block, a.block_size, a.code_phase_uniform,
                       a.pcm_aligned16 != 0, (reinterpret_cast<uintptr_t>(a.pcm) & 15u) == 0, a.stream_stores != 0});
  int32_t *residual = nullptr;
  if (p.residual_bytes != 0) {
    if (!scratch_reserve(ctx, &ctx->d_residual, &ctx->residual_capacity, p.residual_bytes, "hipMalloc residual scratch")) return AAD_APIRESULT_NG;
    residual = ctx->d_residual;
  }
  switch (a.bits) {
    case 4: launch_decode<4>(a, p, residual, ctx->stream); break;
    case 3: launch_decode<3>(a, p, residual, ctx->stream); break;
    default: launch_decode<2>(a, p, residual, ctx->stream); break;
  }
  return hip_ok(ctx, hipGetLastError(), "decode launch") ? AAD_APIRESULT_OK : AAD_APIRESULT_NG;
}

void staging_pool_stop(AADHipContext *ctx)
{
  StagingPool *p = ctx->pool;
  if (p == nullptr) return;
  {
    std::lock_guard<std::mutex> g(p->lock);
    p->stop = true;
  }
  p->work.notify_all();
  for (auto &t : p->threads) t.join();
  delete p;
  ctx->pool = nullptr;
}

int32_t option_from_env(const char *name, const char *const *words, int32_t count)
{
  const char *e = getenv(name);
  if (e == nullptr) return 0;
  for (int32_t i = 0; i < count; i++)
    if (strcmp(e, words[i]) == 0) return i;
  return 0;
}

} /* namespace */

extern "C" {

int32_t AADHip_GetDeviceCount(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

AADApiResult AADHip_ContextCreate(int32_t device_index, void *hip_stream, struct AADHipContext **context)
{
  if (context == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  *context = nullptr;
  if (device_index < 0 || device_index >= AADHip_GetDeviceCount()) return AAD_APIRESULT_NG;
  AADHipContext *ctx = new (std::nothrow) AADHipContext();
  if (ctx == nullptr) return AAD_APIRESULT_NG;
  ctx->device = device_index;
  ctx->stream = static_cast<hipStream_t>(hip_stream);
  ctx->owns_stream = false;
  ctx->last_error[0] = 0;
  ctx->have_events = false;
  ctx->have_pipeline = false;
  ctx->d_scratch = nullptr;
  ctx->scratch_capacity = 0;
  ctx->d_rc_in = ctx->d_rc_out = nullptr;
  ctx->rc_in_capacity = ctx->rc_out_capacity = 0;
  ctx->d_residual = nullptr;
  ctx->residual_capacity = 0;
  ctx->d_trial = nullptr;
  ctx->trial_capacity = 0;
  ctx->d_window_images = nullptr;
  ctx->window_images_capacity = 0;
  ctx->signal_next = aad::LaunchSignal{nullptr, nullptr};
  ctx->pool = nullptr;
  ctx->staging_threads = 0;
  ctx->tile_bytes = 0;
  ctx->d_state = nullptr;
  ctx->state_capacity = 0;
  /* the environment is consulted here (and when the legacy API takes a parked context back into
   * use), never on a launch path */
  AADHipInternal_ContextOptionsFromEnvironment(ctx);
  DeviceGuard guard(ctx);
  int cus = 0, lds_per_cu = 0;
  if (!guard.ok || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_index) != hipSuccess ||
      hipDeviceGetAttribute(&lds_per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device_index) != hipSuccess) {
    delete ctx;
    return AAD_APIRESULT_NG;
  }
  ctx->device_info = aad::Device{(uint32_t)cus, (uint32_t)lds_per_cu};
  if (hip_stream == nullptr) {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      return AAD_APIRESULT_NG;
    }
    ctx->owns_stream = true;
  }
  *context = ctx;
  return AAD_APIRESULT_OK;
}

void AADHip_ContextDestroy(struct AADHipContext *ctx)
{
  if (ctx == nullptr) return;
  staging_pool_stop(ctx);
  {
    DeviceGuard guard(ctx);
    if (guard.ok) {
      (void)hipStreamSynchronize(ctx->stream);
      for (int b = 0; b < 2; b++) {
        staging_release(ctx->in[b]);
        staging_release(ctx->out[b]);
        if (ctx->have_events) (void)hipEventDestroy(ctx->chunk_done[b]);
        if (ctx->have_events && b == 0)
          for (int i = 0; i < 3; i++) (void)hipEventDestroy(ctx->piece_done[i]);
        if (ctx->have_pipeline) {
          (void)hipEventDestroy(ctx->uploaded[b]);
          (void)hipEventDestroy(ctx->computed[b]);
        }
      }
      if (ctx->have_pipeline) {
        (void)hipStreamDestroy(ctx->up_stream);
        (void)hipStreamDestroy(ctx->down_stream);
      }
      if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
      if (ctx->d_rc_in) (void)hipFree(ctx->d_rc_in);
      if (ctx->d_rc_out) (void)hipFree(ctx->d_rc_out);
      if (ctx->d_residual) (void)hipFree(ctx->d_residual);
      if (ctx->d_trial) (void)hipFree(ctx->d_trial);
      if (ctx->d_window_images) (void)hipFree(ctx->d_window_images);
      if (ctx->d_state) (void)hipFree(ctx->d_state);
      if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    }
  }
  delete ctx;
}

AADApiResult AADHip_ContextSynchronize(struct AADHipContext *ctx)
{
  if (ctx == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  DeviceGuard guard(ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  return hip_ok(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize") ? AAD_APIRESULT_OK : AAD_APIRESULT_NG;
}

const char *AADHip_ContextLastError(const struct AADHipContext *ctx) { return ctx ? ctx->last_error : ""; }

void AADHipInternal_ContextOptionsFromEnvironment(struct AADHipContext *ctx)
{
  static const char *const kMappings[] = {"auto", "dense", "quad", "quad-fused", "dense-tiled"};
  static const char *const kTrialLanes[] = {"dual", "single"};
  ctx->signal_refused = AADHip_SignalNextRunSupported() == 0;
  ctx->knobs.lane_mapping = option_from_env("AAD_HIP_MAPPING", kMappings, 5);
  ctx->knobs.trial_lanes = option_from_env("AAD_HIP_TRIAL_LANES", kTrialLanes, 2);
  /* measurement aids */
  const char *ring = getenv("AAD_HIP_ENCODE_RING"), *enc_pad = getenv("AAD_HIP_ENCODE_LDS_PAD");
  const char *dec_pad = getenv("AAD_HIP_DECODE_LDS_PAD"), *nt_min = getenv("AAD_HIP_DECODE_NT_MIN");
  ctx->knobs.encode_ring = ring != nullptr && ring[0] == '0' ? 0 : (ring != nullptr && ring[0] == '2' ? 2 : 1);
  ctx->knobs.encode_lds_pad = enc_pad ? atoi(enc_pad) : -1;
  ctx->knobs.decode_lds_pad = dec_pad ? atoi(dec_pad) : -1;
  ctx->knobs.decode_nt_min = nt_min ? (uint64_t)atoll(nt_min) : 0ull;
  static const char *const kCompareOrders[] = {"auto", "sequential"};
  ctx->compare_sequential = option_from_env("AAD_HIP_COMPARE_ORDER", kCompareOrders, 2);
  const char *threads = getenv("AAD_HIP_STAGING_THREADS");
  if (threads != nullptr && threads[0] >= '1' && threads[0] <= '8' && threads[1] == '\0') ctx->staging_threads = threads[0] - '0';
  const char *tile = getenv("AAD_HIP_TILE_KBYTES");
  if (tile != nullptr) {
    const long long v = atoll(tile);
    if (v > 0 && v <= 0x7FFFFFFF) ctx->tile_bytes = (int64_t)v << 10;
  }
}

int32_t AADHipInternal_ContextDevice(const struct AADHipContext *ctx) { return ctx->device; }

/* ROC_SYSTEM_SCOPE_SIGNAL=0 makes the ROCm runtime give kernel dispatches DEVICE-scope completion signals.  The events of
 * AADHip_ContextSignalNextRun ARE the kernel's completion signal (hipExtLaunchKernelGGL's stop event), and a wait on one
 * from another queue (hipStreamWaitEvent on a second stream: the two-stream pipeline of bench.py / EncodeDecodePipeline)
 * then never returns - recorded in tools/experiments/README.md ("runtime knobs") and gpurun_out/runtime_knobs.txt of round 3.
 * The library does not try to work under that setting: it says no. */
int32_t AADHip_SignalNextRunSupported(void)
{
  const char *v = getenv("ROC_SYSTEM_SCOPE_SIGNAL");
  return (v != nullptr && v[0] == '0' && v[1] == '\0') ? 0 : 1;
}

AADApiResult AADHip_ContextSignalNextRun(struct AADHipContext *ctx, void *hip_start_event, void *hip_stop_event)
{
  if (ctx == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  if (ctx->signal_refused && (hip_start_event != nullptr || hip_stop_event != nullptr)) {
    snprintf(ctx->last_error, sizeof(ctx->last_error),
             "AADHip_ContextSignalNextRun: refused, ROC_SYSTEM_SCOPE_SIGNAL=0 (device-scope completion signals: a wait on the "
             "run's event from another stream would never return); record an event behind the run instead");
    return AAD_APIRESULT_NG;
  }
  ctx->signal_next = aad::LaunchSignal{static_cast<hipEvent_t>(hip_start_event), static_cast<hipEvent_t>(hip_stop_event)};
  return AAD_APIRESULT_OK;
}

AADApiResult AADHip_ContextSetOption(struct AADHipContext *ctx, int32_t option, int32_t value)
{
  if (ctx == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  switch (option) {
    case AAD_HIP_OPTION_LANE_MAPPING:
      if (value < AAD_HIP_LANE_MAPPING_AUTO || value > AAD_HIP_LANE_MAPPING_DENSE_TILED) return AAD_APIRESULT_INVALID_ARGUMENT;
      ctx->knobs.lane_mapping = value;
      return AAD_APIRESULT_OK;
    case AAD_HIP_OPTION_TRIAL_LANES:
      if (value != AAD_HIP_TRIAL_LANES_DUAL && value != AAD_HIP_TRIAL_LANES_SINGLE) return AAD_APIRESULT_INVALID_ARGUMENT;
      ctx->knobs.trial_lanes = value;
      return AAD_APIRESULT_OK;
    case AAD_HIP_OPTION_SIMD_ROLE:
      if (value < AAD_HIP_SIMD_ROLE_OFF || value > AAD_HIP_SIMD_ROLE_3) return AAD_APIRESULT_INVALID_ARGUMENT;
      ctx->knobs.simd_role = value;
      return AAD_APIRESULT_OK;
    case AAD_HIP_OPTION_COMPARE_ORDER:
      if (value != 0 && value != 1) return AAD_APIRESULT_INVALID_ARGUMENT;
      ctx->compare_sequential = value;
      return AAD_APIRESULT_OK;
    case AAD_HIP_OPTION_STAGING_THREADS:
      if (value < 0 || value > 8) return AAD_APIRESULT_INVALID_ARGUMENT;
      ctx->staging_threads = value;
      return AAD_APIRESULT_OK;
    case AAD_HIP_OPTION_TILE_KBYTES:
      if (value < 0) return AAD_APIRESULT_INVALID_ARGUMENT;
      ctx->tile_bytes = (int64_t)value << 10;
      return AAD_APIRESULT_OK;
    default:
      return AAD_APIRESULT_INVALID_ARGUMENT;
  }
}

uint64_t AADHip_CalculateEncodedSize(const struct AADEncodeParameter *parameter, uint32_t num_samples)
{
  AADHeaderInfo h;
  if (num_samples == 0) return 0;
  if (AADFormat_ParameterToHeader(parameter, num_samples, AAD_HIP_MAX_NUM_CHANNELS, &h) != AAD_APIRESULT_OK) return 0;
  if (!AADFormat_HeaderFieldsValid(&h, AAD_HIP_MAX_NUM_CHANNELS)) return 0;
  return AADFormat_EncodedSize(&h);
}

/* ------------------------------------------------------------------------------- encode -- */

AADApiResult AADHip_EncodePlanCreate(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                     uint32_t num_streams, const struct AADHipStreamDesc *streams,
                                     struct AADHipEncodePlan **plan)
{
  if (ctx == nullptr || parameter == nullptr || plan == nullptr || (num_streams != 0 && streams == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  return encode_plan_create(ctx, parameter, nullptr, nullptr, nullptr, num_streams, streams, plan);
}

void AADHip_EncodePlanDestroy(struct AADHipEncodePlan *plan)
{
  if (plan == nullptr) return;
  DeviceGuard guard(plan->ctx);
  if (guard.ok) {
    (void)hipStreamSynchronize(plan->ctx->stream);
    (void)hipFree(plan->d_table);
    (void)hipFree(plan->d_out_base);
    (void)hipFree(plan->d_stats_stream);
    if (plan->windows != nullptr) {
      (void)hipFree(plan->windows->d_sources);
      if (plan->windows->d_lanes) (void)hipFree(plan->windows->d_lanes);
    }
  }
  delete plan->windows;
  delete plan;
}

AADApiResult AADHip_SegmentedEncodePlanCreate(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                              const struct AADHipSegmentation *segmentation, uint32_t num_streams,
                                              const struct AADHipStreamDesc *streams, struct AADHipEncodePlan **plan)
{
  if (ctx == nullptr || parameter == nullptr || segmentation == nullptr || plan == nullptr || (num_streams != 0 && streams == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  if (segmentation->segment_blocks == 0) return AAD_APIRESULT_INVALID_ARGUMENT;
  return encode_plan_create(ctx, parameter, nullptr, nullptr, segmentation, num_streams, streams, plan);
}

AADApiResult AADHip_EncodePlanRun(struct AADHipEncodePlan *plan, const int16_t *device_pcm, uint8_t *device_data,
                                  struct AADHipLaneState *device_state)
{
  return encode_plan_run(plan, EncodePlanKind::Frames, device_pcm, device_data, nullptr, device_state);
}

/* ------------------------------------------------------------------------ planar encode -- */

AADApiResult AADHip_PlanarEncodePlanCreate(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                           const struct AADHipPlanarLayout *layout, const struct AADHipSegmentation *segmentation,
                                           uint32_t num_streams, const struct AADHipStreamDesc *streams, struct AADHipEncodePlan **plan)
{
  if (ctx == nullptr || parameter == nullptr || layout == nullptr || plan == nullptr || (num_streams != 0 && streams == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  if (!planar_fields_ok(layout, segmentation)) return AAD_APIRESULT_INVALID_ARGUMENT;
  return encode_plan_create(ctx, parameter, layout, nullptr, segmentation, num_streams, streams, plan);
}

AADApiResult AADHip_PlanarEncodePlanRun(struct AADHipEncodePlan *plan, const void *device_samples, uint8_t *device_data,
                                        struct AADHipLaneState *device_state)
{
  return encode_plan_run(plan, EncodePlanKind::Rows, device_samples, device_data, nullptr, device_state);
}

/* ------------------------------------------------------------------ planar reconstruct -- */

AADApiResult AADHip_PlanarReconstructPlanCreate(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                                const struct AADHipPlanarLayout *input, const struct AADHipPlanarOutput *output,
                                                const struct AADHipSegmentation *segmentation, uint32_t num_streams,
                                                const struct AADHipStreamDesc *streams, struct AADHipEncodePlan **plan)
{
  if (ctx == nullptr || output == nullptr || plan == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  if (parameter == nullptr || input == nullptr || (num_streams != 0 && streams == nullptr)) return AAD_APIRESULT_INVALID_ARGUMENT;
  if (!planar_fields_ok(input, segmentation)) return AAD_APIRESULT_INVALID_ARGUMENT;
  return encode_plan_create(ctx, parameter, input, output, segmentation, num_streams, streams, plan);
}

AADApiResult AADHip_PlanarReconstructPlanRun(struct AADHipEncodePlan *plan, const void *device_samples, uint8_t *device_data,
                                             void *device_out, struct AADHipLaneState *device_state)
{
  return encode_plan_run(plan, EncodePlanKind::Reconstruct, device_samples, device_data, device_out, device_state);
}

AADApiResult AADHip_PlanarReconstructPlanRunStats(struct AADHipEncodePlan *plan, const void *device_samples, uint8_t *device_data,
                                                  void *device_out, struct AADHipLaneState *device_state,
                                                  struct AADHipRowStats *device_stats)
{
  return encode_plan_run(plan, EncodePlanKind::Reconstruct, device_samples, device_data, device_out, device_state, true, device_stats);
}

/* ------------------------------------------------------------------------------- decode -- */

AADApiResult AADHip_DecodePlanCreate(struct AADHipContext *ctx, const struct AADHeaderInfo *format,
                                     int32_t has_file_header, uint32_t num_streams,
                                     const struct AADHipStreamDesc *streams, struct AADHipDecodePlan **plan)
{
  if (ctx == nullptr || format == nullptr || plan == nullptr || (num_streams != 0 && streams == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  std::vector<uint64_t> prefix((size_t)num_streams + 1);
  aad::DecodeArgs args;
  const AADApiResult rc = decode_plan_init(format, has_file_header, num_streams, streams, prefix.data(), &args);
  if (rc != AAD_APIRESULT_OK) return rc;

  AADHipDecodePlan *p = new (std::nothrow) AADHipDecodePlan();
  if (p == nullptr) return AAD_APIRESULT_NG;
  p->ctx = ctx;
  p->d_streams = nullptr;
  p->d_prefix = nullptr;
  DeviceGuard guard(ctx);
  if (!guard.ok || !upload(ctx, &p->d_streams, reinterpret_cast<const aad::StreamDesc *>(streams), num_streams) ||
      !upload(ctx, &p->d_prefix, prefix.data(), prefix.size())) {
    if (p->d_streams) (void)hipFree(p->d_streams);
    if (p->d_prefix) (void)hipFree(p->d_prefix);
    delete p;
    return AAD_APIRESULT_NG;
  }
  p->args = args;
  p->args.streams = p->d_streams;
  p->args.block_prefix = p->d_prefix;
  *plan = p;
  return AAD_APIRESULT_OK;
}

void AADHip_DecodePlanDestroy(struct AADHipDecodePlan *plan)
{
  if (plan == nullptr) return;
  DeviceGuard guard(plan->ctx);
  if (guard.ok) {
    (void)hipStreamSynchronize(plan->ctx->stream);
    (void)hipFree(plan->d_streams);
    (void)hipFree(plan->d_prefix);
  }
  delete plan;
}

AADApiResult AADHip_DecodePlanRun(struct AADHipDecodePlan *plan, const uint8_t *device_data, int16_t *device_pcm)
{
  if (plan == nullptr || device_data == nullptr || device_pcm == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  AADHipContext *ctx = plan->ctx;
  const aad::LaunchSignal signal = take_signal(ctx);
  DeviceGuard guard(ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  if (plan->args.total_blocks == 0) return finish_signal(ctx, signal, AAD_APIRESULT_OK);
  aad::DecodeArgs a = plan->args;
  a.data = device_data;
  a.pcm = device_pcm;
  if ((reinterpret_cast<uintptr_t>(device_pcm) & 63u) != 0) a.stream_stores = 0;
  aad::tl_launch_signal = signal;
  return finish_signal(ctx, signal, run_decode(ctx, a));
}

/* ------------------------------------------------------------------------- window decode -- */

static_assert(sizeof(AADHipWindow) == 2 * sizeof(uint64_t), "window table layout");

namespace {
/* What the three creates share, behind their validation: the plan with its descriptor table and, where the kind has them, its
 * format records (records: num_streams of them, record_bytes each, or null) in device memory */
AADApiResult window_plan_create(AADHipContext *ctx, aad::WindowKind kind, const aad::DecodeArgs &args, const aad::WindowVariants &variants,
                                const struct AADHipStreamDesc *streams, const void *records, size_t record_bytes,
                                struct AADHipWindowDecodePlan **plan)
{
  AADHipWindowDecodePlan *p = new (std::nothrow) AADHipWindowDecodePlan();
  if (p == nullptr) return AAD_APIRESULT_NG;
  p->ctx = ctx;
  p->kind = kind;
  p->variants = variants;
  uint8_t *d_records = nullptr;
  DeviceGuard guard(ctx);
  const bool ok = guard.ok && upload(ctx, &p->d_streams, reinterpret_cast<const aad::StreamDesc *>(streams), args.num_streams) &&
                  (records == nullptr || upload(ctx, &d_records, static_cast<const uint8_t *>(records), record_bytes * args.num_streams));
  if (!ok) {
    if (p->d_streams) (void)hipFree(p->d_streams);
    if (d_records) (void)hipFree(d_records);
    delete p;
    return AAD_APIRESULT_NG;
  }
  p->d_formats = d_records;
  p->args = args;
  p->args.streams = p->d_streams;
  *plan = p;
  return AAD_APIRESULT_OK;
}

/* `args` of a plan whose formats come per stream */
aad::DecodeArgs window_plan_args(uint32_t num_streams, uint32_t channels, int32_t has_file_header)
{
  aad::DecodeArgs args;
  memset(&args, 0, sizeof(args));
  args.num_streams = num_streams;
  args.channels = channels;
  args.header_bytes = has_file_header ? AAD_HEADER_SIZE : 0;
  return args;
}

/* stream i of such a plan: what AADHip_DecodePlanCreate checks of its one format and table */
AADApiResult window_plan_stream_check(const struct AADHeaderInfo *format, int32_t has_file_header, const struct AADHipStreamDesc *stream)
{
  uint64_t prefix[2];
  aad::DecodeArgs one;
  return decode_plan_init(format, has_file_header, 1, stream, prefix, &one);
}
} /* namespace */

AADApiResult AADHip_WindowDecodePlanCreate(struct AADHipContext *ctx, const struct AADHeaderInfo *format, int32_t has_file_header,
                                           uint32_t num_streams, const struct AADHipStreamDesc *streams,
                                           struct AADHipWindowDecodePlan **plan)
{
  if (ctx == nullptr || format == nullptr || plan == nullptr || (num_streams != 0 && streams == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  std::vector<uint64_t> prefix((size_t)num_streams + 1);
  aad::DecodeArgs args;
  const AADApiResult rc = decode_plan_init(format, has_file_header, num_streams, streams, prefix.data(), &args);
  if (rc != AAD_APIRESULT_OK) return rc;
  const aad::WindowVariants one = {1, {{args.channels, args.bits, args.mid_side, args.samples_per_block, num_streams}}};
  return window_plan_create(ctx, aad::WindowKind::Same, args, one, streams, nullptr, 0, plan);
}

AADApiResult AADHip_MixedWindowDecodePlanCreate(struct AADHipContext *ctx, uint32_t num_channels, int32_t has_file_header,
                                                uint32_t num_streams, const struct AADHipStreamDesc *streams,
                                                const struct AADHeaderInfo *formats, struct AADHipWindowDecodePlan **plan)
{
  if (ctx == nullptr || plan == nullptr || (num_streams != 0 && (streams == nullptr || formats == nullptr)))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  if (num_channels < 1 || num_channels > AAD_HIP_MAX_NUM_CHANNELS) return AAD_APIRESULT_INVALID_ARGUMENT;
  /* stream by stream; the first failing stream's error */
  std::vector<aad::StreamFormat> records(num_streams);
  for (uint32_t i = 0; i < num_streams; i++) {
    if (formats[i].num_channels != num_channels) return AAD_APIRESULT_INVALID_ARGUMENT;
    const AADApiResult rc = window_plan_stream_check(&formats[i], has_file_header, &streams[i]);
    if (rc != AAD_APIRESULT_OK) return rc;
    records[i] = aad::stream_format_of(formats[i], num_channels);
  }
  return window_plan_create(ctx, aad::WindowKind::Mixed, window_plan_args(num_streams, num_channels, has_file_header),
                            aad::window_variants(records.data(), num_streams), streams, records.data(), sizeof(records[0]), plan);
}

AADApiResult AADHip_ChannelMixWindowDecodePlanCreate(struct AADHipContext *ctx, uint32_t out_channels, int32_t has_file_header,
                                                     uint32_t num_streams, const struct AADHipStreamDesc *streams,
                                                     const struct AADHeaderInfo *formats, struct AADHipWindowDecodePlan **plan)
{
  if (ctx == nullptr || plan == nullptr || (num_streams != 0 && (streams == nullptr || formats == nullptr)))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  if (out_channels < 1 || out_channels > 2) return AAD_APIRESULT_INVALID_ARGUMENT;
  std::vector<aad::ChannelStreamFormat> records(num_streams);
  for (uint32_t i = 0; i < num_streams; i++) {
    if (formats[i].num_channels < 1 || formats[i].num_channels > 2) return AAD_APIRESULT_INVALID_ARGUMENT;
    const AADApiResult rc = window_plan_stream_check(&formats[i], has_file_header, &streams[i]);
    if (rc != AAD_APIRESULT_OK) return rc;
    records[i] = aad::channel_stream_format_of(formats[i]);
  }
  return window_plan_create(ctx, aad::WindowKind::ChannelMix, window_plan_args(num_streams, out_channels, has_file_header),
                            aad::channel_mix_variants(records.data(), num_streams), streams, records.data(), sizeof(records[0]), plan);
}

void AADHip_WindowDecodePlanDestroy(struct AADHipWindowDecodePlan *plan)
{
  if (plan == nullptr) return;
  DeviceGuard guard(plan->ctx);
  if (guard.ok) {
    (void)hipStreamSynchronize(plan->ctx->stream);
    (void)hipFree(plan->d_streams);
    if (plan->d_formats) (void)hipFree(plan->d_formats);
  }
  delete plan;
}

namespace {
/* AADHip_WindowDecodePlanRunGain's part of a run: the launches are the gain units' (aad_launch.h WindowMode) */
struct WindowGainRun {
  bool on;
  const float *gain; /* device memory, or null: every gain is 1 */
  uint32_t add;
};
/* AADHip_WindowDecodePlanRunPlaced's / ...RunPlacedStats' part of a run: the launches are the placed units' (WindowMode) - the
 * gain units' rows or the statistics alone, each window's crop clipped to and placed by its span */
struct WindowPlacedRun {
  bool on;
  const struct AADHipWindowSpan *spans; /* device memory, or null: every span is (T, 0) */
};

/* AADHip_WindowDecodePlanRunStats: the lanes add into the table, so the run clears it in front of its first launch - the start
 * event recorded in front of the clear, and the launches carry the stop event alone (as a segmented reconstruct's statistics) */
bool clear_window_stats(AADHipContext *ctx, aad::LaunchSignal *signal, struct AADHipRowStats *stats, uint64_t bytes)
{
  if (signal->start != nullptr && !hip_ok(ctx, hipEventRecord(signal->start, ctx->stream), "hipEventRecord")) return false;
  signal->start = nullptr;
  return hip_ok(ctx, hipMemsetAsync(stats, 0, bytes, ctx->stream), "hipMemsetAsync");
}

/* Every run of every kind of plan.  AADHip_WindowDecodePlanRun, and with_stats AADHip_WindowDecodePlanRunStats (stats_bytes
 * below: the table's size): the table as a further output, device_out optional;
 * gain.on: AADHip_WindowDecodePlanRunGain, float rows alone, `mode` its STORE / ADD argument as the caller gave it;
 * placed.on: with gain.on AADHip_WindowDecodePlanRunPlaced, with_stats (and no rows) AADHip_WindowDecodePlanRunPlacedStats */
AADApiResult window_decode_run(struct AADHipWindowDecodePlan *plan, const uint8_t *device_data, uint64_t num_windows,
                               const struct AADHipWindow *device_windows, uint32_t frames_per_window, int32_t sample_type,
                               void *device_out, bool with_stats, struct AADHipRowStats *stats,
                               WindowGainRun gain = WindowGainRun{false, nullptr, 0}, int32_t mode = 0,
                               WindowPlacedRun placed = WindowPlacedRun{false, nullptr})
{
  if (plan == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  AADHipContext *ctx = plan->ctx;
  aad::LaunchSignal signal = take_signal(ctx);
  if (gain.on) {
    if (sample_type == AAD_HIP_SAMPLE_INT16 || (mode != AAD_HIP_WINDOW_GAIN_STORE && mode != AAD_HIP_WINDOW_GAIN_ADD) ||
        (reinterpret_cast<uintptr_t>(gain.gain) & 3u) != 0) {
      snprintf(ctx->last_error, sizeof(ctx->last_error),
               "window decode with gain: int16 rows, a mode that is neither STORE nor ADD, or a gain table off 4-byte alignment");
      return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
    }
    gain.add = mode == AAD_HIP_WINDOW_GAIN_ADD;
  }
  if (placed.on && (reinterpret_cast<uintptr_t>(placed.spans) & 7u) != 0) {
    snprintf(ctx->last_error, sizeof(ctx->last_error), "window decode with spans: a span table off 8-byte alignment");
    return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  }
  if (frames_per_window == 0 || !window_sample_type_ok(sample_type) ||
      (num_windows != 0 && (device_data == nullptr || device_windows == nullptr || (device_out == nullptr && !with_stats))))
    return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  uint64_t stats_bytes = 0;
  if (with_stats) {
    const aad::WindowStatsTable t = aad::window_stats_table(num_windows, plan->args.channels, (uint64_t)reinterpret_cast<uintptr_t>(stats));
    if (!t.ok) {
      snprintf(ctx->last_error, sizeof(ctx->last_error),
               "window decode statistics: a null or unaligned table, or %llu windows x %u channels x 32 bytes overflow 64 bits",
               (unsigned long long)num_windows, plan->args.channels);
      return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
    }
    stats_bytes = t.bytes;
  } else {
    stats = nullptr;
  }
  const aad::DecodeArgs &d = plan->args;
  const aad::WindowRunPlan m =
      aad::plan_window_run(ctx->device_info, ctx->knobs, plan->kind, plan->variants, num_windows, frames_per_window, d.channels);
  if (!m.ok) {
    snprintf(ctx->last_error, sizeof(ctx->last_error), "window decode: %llu windows x %u channels x %u frames overflow 64 bits",
             (unsigned long long)num_windows, d.channels, frames_per_window);
    return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  }
  DeviceGuard guard(ctx);
  if (!guard.ok) return finish_signal(ctx, signal, AAD_APIRESULT_NG);
  if (num_windows == 0) return finish_signal(ctx, signal, AAD_APIRESULT_OK);
  /* a same-format plan's header may name bits no kernel decodes; the formats of the other kinds were checked stream by stream */
  if (m.variant[0].bits < 2 || m.variant[0].bits > 4) return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_FORMAT);
  if (stats != nullptr && !clear_window_stats(ctx, &signal, stats, stats_bytes)) return finish_signal(ctx, signal, AAD_APIRESULT_NG);
  const aad::WindowMode unit_mode = placed.on && stats != nullptr ? aad::WindowMode::PlacedStats
                                    : placed.on                   ? aad::WindowMode::Placed
                                    : stats != nullptr            ? aad::WindowMode::Stats
                                    : gain.on                     ? aad::WindowMode::Gain
                                                                  : aad::WindowMode::Rows;
  static const char *const launch_name[] = {"window decode launch", "mixed window decode launch", "channel-mix window decode launch"};
  /* The launches of the run, in the stream's order: one per kernel variant of the plan, each over all the windows.  The start
   * event rides on the first and the stop event on the last (aad_launch.h); a plan with one variant is one kernel */
  aad::LaunchSignal last = signal;
  for (uint32_t i = 0; i < m.count; i++) {
    aad::WindowArgs a;
    memset(&a, 0, sizeof(a));
    a.streams = d.streams;
    a.data = device_data;
    a.windows = reinterpret_cast<const uint64_t *>(device_windows);
    a.out = device_out;
    a.lanes = m.launch[i].lanes;
    a.blocks_per_window = m.launch[i].blocks_per_window;
    a.frames = frames_per_window;
    a.num_streams = d.num_streams;
    a.channels = m.variant[i].channels;
    a.block_size = d.block_size; /* 0 but in a same-format plan: the other kernels read their stream's record */
    a.samples_per_block = m.variant[i].min_samples_per_block;
    a.header_bytes = d.header_bytes;
    a.mid_side = m.variant[i].mid_side;
    a.bits = m.variant[i].bits;
    const aad::WindowUnitRun run = {a, plan->d_formats, i == 0, d.channels, gain.gain, gain.add, placed.spans, stats};
    last = aad::LaunchSignal{i == 0 ? signal.start : nullptr, i + 1 == m.count ? signal.stop : nullptr};
    aad::tl_launch_signal = last;
    aad::launch_window_unit(plan->kind, unit_mode, run, m.launch[i], sample_type, ctx->stream);
    if (!hip_ok(ctx, hipGetLastError(), launch_name[(uint32_t)plan->kind])) return finish_signal(ctx, signal, AAD_APIRESULT_NG);
  }
  return finish_signal(ctx, last, AAD_APIRESULT_OK);
}
} /* namespace */

AADApiResult AADHip_WindowDecodePlanRun(struct AADHipWindowDecodePlan *plan, const uint8_t *device_data, uint64_t num_windows,
                                        const struct AADHipWindow *device_windows, uint32_t frames_per_window, int32_t sample_type,
                                        void *device_out)
{
  return window_decode_run(plan, device_data, num_windows, device_windows, frames_per_window, sample_type, device_out, false, nullptr);
}

AADApiResult AADHip_WindowDecodePlanRunStats(struct AADHipWindowDecodePlan *plan, const uint8_t *device_data, uint64_t num_windows,
                                             const struct AADHipWindow *device_windows, uint32_t frames_per_window,
                                             int32_t sample_type, void *device_out, struct AADHipRowStats *device_stats)
{
  return window_decode_run(plan, device_data, num_windows, device_windows, frames_per_window, sample_type, device_out, true,
                           device_stats);
}

AADApiResult AADHip_WindowDecodePlanRunGain(struct AADHipWindowDecodePlan *plan, const uint8_t *device_data, uint64_t num_windows,
                                            const struct AADHipWindow *device_windows, uint32_t frames_per_window,
                                            int32_t sample_type, void *device_out, const float *device_gain, int32_t mode)
{
  return window_decode_run(plan, device_data, num_windows, device_windows, frames_per_window, sample_type, device_out, false, nullptr,
                           WindowGainRun{true, device_gain, 0}, mode);
}

AADApiResult AADHip_WindowDecodePlanRunPlaced(struct AADHipWindowDecodePlan *plan, const uint8_t *device_data, uint64_t num_windows,
                                              const struct AADHipWindow *device_windows, const struct AADHipWindowSpan *device_spans,
                                              uint32_t frames_per_window, int32_t sample_type, void *device_out,
                                              const float *device_gain, int32_t mode)
{
  return window_decode_run(plan, device_data, num_windows, device_windows, frames_per_window, sample_type, device_out, false, nullptr,
                           WindowGainRun{true, device_gain, 0}, mode, WindowPlacedRun{true, device_spans});
}

/* no rows: the sample type is of no account, and window_decode_run sees the statistics run of int16 rows that are not there */
AADApiResult AADHip_WindowDecodePlanRunPlacedStats(struct AADHipWindowDecodePlan *plan, const uint8_t *device_data,
                                                   uint64_t num_windows, const struct AADHipWindow *device_windows,
                                                   const struct AADHipWindowSpan *device_spans, uint32_t frames_per_window,
                                                   struct AADHipRowStats *device_stats)
{
  return window_decode_run(plan, device_data, num_windows, device_windows, frames_per_window, AAD_HIP_SAMPLE_INT16, nullptr, true,
                           device_stats, WindowGainRun{false, nullptr, 0}, 0, WindowPlacedRun{true, device_spans});
}

/* -------------------------------------------------------------------- window reconstruct -- */

AADApiResult AADHip_WindowReconstructPlanCreate(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                                const struct AADHipPlanarLayout *input, const struct AADHipSegmentation *segmentation,
                                                uint32_t num_source_streams, const struct AADHipStreamDesc *source_streams,
                                                struct AADHipEncodePlan **plan)
{
  if (ctx == nullptr || plan == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  if (parameter == nullptr || input == nullptr || (num_source_streams != 0 && source_streams == nullptr)) return AAD_APIRESULT_INVALID_ARGUMENT;
  if (!planar_fields_ok(input, segmentation)) return AAD_APIRESULT_INVALID_ARGUMENT;
  aad::EncodeRun run;
  const AADApiResult rc = encode_plan_init(parameter, 0, nullptr, &run.args);
  if (rc != AAD_APIRESULT_OK) return rc;
  if (!aad::window_sources_ok(run.args.channels, input->channel_stride, input->sample_type == AAD_HIP_SAMPLE_FLOAT32 ? 4u : 2u,
                              num_source_streams, source_streams)) {
    snprintf(ctx->last_error, sizeof(ctx->last_error),
             "window reconstruct plan: source rows refused (channel_stride below a stream's num_samples, or past 64-bit offsets)");
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  AADHipEncodePlan *p = new (std::nothrow) AADHipEncodePlan(); /* every table pointer null */
  WindowPlanPart *part = new (std::nothrow) WindowPlanPart();
  if (p == nullptr || part == nullptr) {
    delete p;
    delete part;
    return AAD_APIRESULT_NG;
  }
  p->ctx = ctx;
  p->kind = EncodePlanKind::Windows;
  p->windows = part;
  part->seg = segmentation != nullptr ? *segmentation : AADHipSegmentation{0, 0};
  part->parameter = *parameter;
  part->num_sources = num_source_streams;
  DeviceGuard guard(ctx);
  if (!guard.ok || !upload(ctx, &part->d_sources, source_streams, num_source_streams)) {
    if (part->d_sources) (void)hipFree(part->d_sources);
    delete part;
    delete p;
    return AAD_APIRESULT_NG;
  }
  run.args.ring_ok = 0; /* the byte ring stores whole sectors, past an image's last byte: a run touches the image bytes alone */
  run.in = aad::planar_layout(input->sample_type, run.args.channels);
  run.channel_stride = input->channel_stride;
  p->run = run;
  *plan = p;
  return AAD_APIRESULT_OK;
}

void AADHip_WindowReconstructPlanDestroy(struct AADHipEncodePlan *plan) { AADHip_EncodePlanDestroy(plan); }

AADApiResult AADHip_WindowReconstructPlanRun(struct AADHipEncodePlan *plan, const void *device_samples, uint64_t num_windows,
                                             const struct AADHipWindow *device_windows, uint32_t frames_per_window,
                                             uint64_t image_stride, uint8_t *device_data, const struct AADHipPlanarOutput *output,
                                             void *device_out, struct AADHipRowStats *device_stats)
{
  if (plan == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  AADHipContext *ctx = plan->ctx;
  const aad::LaunchSignal signal = take_signal(ctx);
  auto refuse = [&](const char *why) {
    snprintf(ctx->last_error, sizeof(ctx->last_error), "window reconstruct: %s", why);
    return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_ARGUMENT);
  };
  if (plan->kind != EncodePlanKind::Windows) return refuse("not a window reconstruct plan");
  WindowPlanPart *part = plan->windows;
  const aad::EncodeArgs &e = plan->run.args;
  if (frames_per_window == 0) return refuse("frames_per_window == 0");
  if (num_windows != 0 && device_data == nullptr && device_out == nullptr && device_stats == nullptr)
    return refuse("no output: images, rows and statistics are all null");
  if (device_out != nullptr && !aad::planar_output_rows_ok(e.channels, num_windows, frames_per_window, output))
    return refuse("output rows refused (null, sample type, reserved, a stride below the rows of T elements, or past 64-bit offsets)");
  if (device_out != nullptr && device_out == device_samples) return refuse("device_out == device_samples");
  const uint64_t image_bytes = AADHip_CalculateEncodedSize(&part->parameter, frames_per_window);
  if (image_bytes == 0) return finish_signal(ctx, signal, AAD_APIRESULT_INVALID_FORMAT);
  if (device_data == nullptr) image_stride = (image_bytes + 63) / 64 * 64; /* the context's scratch: a layout of its own */
  if (!aad::window_images_ok(num_windows, image_stride, image_bytes))
    return refuse("image_stride below the image of a full window, or images past 64-bit offsets");
  uint64_t lanes = 0;
  if (!aad::window_lane_count(num_windows, frames_per_window, e.samples_per_block, part->seg.segment_blocks, &lanes))
    return refuse("more than UINT32_MAX lanes (windows x chains per window)");
  if (num_windows != 0 && (device_samples == nullptr || device_windows == nullptr || (reinterpret_cast<uintptr_t>(device_windows) & 7u) != 0 ||
                           (reinterpret_cast<uintptr_t>(device_stats) & 7u) != 0))
    return refuse("a null corpus, a null or misaligned window table, or a misaligned statistics table");
  DeviceGuard guard(ctx);
  if (!guard.ok) return finish_signal(ctx, signal, AAD_APIRESULT_NG);
  if (num_windows == 0) return finish_signal(ctx, signal, AAD_APIRESULT_OK);

  const bool segmented = part->seg.segment_blocks != 0;
  const uint64_t entry = segmented ? sizeof(aad::ChainDesc) : sizeof(aad::StreamDesc);
  const uint64_t base_at = lanes * entry, stats_at = base_at + lanes * sizeof(uint64_t); /* 8-byte records first: every table aligned */
  if (!scratch_reserve(ctx, &part->d_lanes, &part->lanes_capacity, stats_at + lanes * sizeof(uint32_t), "hipMalloc window lane tables"))
    return finish_signal(ctx, signal, AAD_APIRESULT_NG);
  if (device_data == nullptr) {
    if (!scratch_reserve(ctx, &ctx->d_window_images, &ctx->window_images_capacity, (num_windows - 1) * image_stride + image_bytes,
                         "hipMalloc window image scratch"))
      return finish_signal(ctx, signal, AAD_APIRESULT_NG);
    device_data = ctx->d_window_images;
  }

  aad::WindowResolveArgs w;
  memset(&w, 0, sizeof(w));
  w.sources = part->d_sources;
  w.windows = reinterpret_cast<const uint64_t *>(device_windows);
  w.num_sources = part->num_sources;
  w.num_windows = num_windows;
  w.g.frames = frames_per_window;
  w.g.spb = e.samples_per_block;
  w.g.segment_blocks = part->seg.segment_blocks;
  w.g.warmup_blocks = part->seg.warmup_blocks;
  w.g.chains_per_window = (uint32_t)(lanes / num_windows);
  w.g.image_stride = image_stride;
  w.g.out_stream_stride = device_out != nullptr ? output->stream_stride : 0;
  w.table = part->d_lanes;
  w.out_base = reinterpret_cast<uint64_t *>(part->d_lanes + base_at);
  w.stats_stream = reinterpret_cast<uint32_t *>(part->d_lanes + stats_at);
  w.out = device_out;
  w.out_channel_stride = device_out != nullptr ? output->channel_stride : 0;
  w.channels = e.channels;
  w.out_float32 = device_out != nullptr && output->sample_type == AAD_HIP_SAMPLE_FLOAT32;

  aad::EncodeRun r = plan->run;
  r.args.num_streams = (uint32_t)lanes;
  if (segmented) use_chain_table(&r, reinterpret_cast<const aad::ChainDesc *>(part->d_lanes), (uint32_t)lanes);
  else r.args.streams = reinterpret_cast<const aad::StreamDesc *>(part->d_lanes);
  r.args.pcm = static_cast<const int16_t *>(device_samples);
  r.args.data = device_data;
  r.rows = aad::RecRows{device_out, w.out_base, w.out_channel_stride};
  r.rec = device_out != nullptr ? aad::rec_output(output->sample_type) : aad::kRecNone;
  if (device_stats != nullptr) {
    r.rec = aad::rec_with_stats(r.rec, device_out != nullptr);
    r.stats = device_stats;
    r.stats_stream = segmented ? w.stats_stream : nullptr;
  }
  /* The run's device operations, in the stream's order: the resolve kernel (which also zeroes the row tails), [the clear of the
   * statistics], the encoders.  The start event rides on the first of them and the stop event on the last (aad_launch.h). */
  aad::tl_launch_signal = aad::LaunchSignal{signal.start, nullptr};
  aad::launch_window_resolve(w, ctx->stream);
  if (!hip_ok(ctx, hipGetLastError(), "window resolve launch")) return finish_signal(ctx, signal, AAD_APIRESULT_NG);
  if (device_stats != nullptr && segmented && /* the chains of a window add into its records */
      !hip_ok(ctx, hipMemsetAsync(device_stats, 0, num_windows * e.channels * sizeof(struct AADHipRowStats), ctx->stream), "hipMemsetAsync"))
    return finish_signal(ctx, signal, AAD_APIRESULT_NG);
  const aad::LaunchSignal stop_only = {nullptr, signal.stop};
  aad::tl_launch_signal = stop_only;
  return finish_signal(ctx, stop_only, run_encode(ctx, r));
}

} /* extern "C" */

/* --------------------------------------------------------------- host-memory calls ----------
 *
 * Call pattern served: the reference CLI's (src/main.c:182-198 encode, :91-106 decode) - host
 * buffers in, host buffers out, synchronous - for one stream (legacy API) or many (AADHip_*Batch).
 *
 * One chunk of streams = one pinned input block {stream table, [block prefix], [state], payload}
 * -> ONE H2D copy -> kernel -> ONE D2H copy of the output block {payload, [state]}.  No hipMalloc,
 * no plan object, no synchronisation besides the wait for the chunk's last copy.  Batches above
 * kChunkBudget bytes are cut into chunks that alternate between two block pairs: the host fills
 * chunk k+1 and drains chunk k-1 while chunk k is on the device (the staging memcpys are the
 * slowest stage of this path - one core moves ~10 GB/s, PCIe ~50 GB/s, the kernels more).
 */
namespace {

using aad::round_up;

constexpr uint64_t kParallelStagingAbove = 1ull << 20; /* bytes in a chunk from which the helper threads pay */

unsigned staging_threads(const AADHipContext *ctx)
{
  if (ctx->staging_threads > 0) return (unsigned)ctx->staging_threads;
  static const unsigned hw = std::thread::hardware_concurrency(); /* asked once: it reads /sys */
  /* round 4 (tools/host_size_sweep.py, 100 000 one-block stereo streams = 0.5 GB per direction): decode 7.9 / 10.9 / 12.0 / 13.6
   * Gsamples/s with 2 / 4 / 6 / 8 copying threads - the drain of 2 bytes per sample into pageable memory is the slowest stage -
   * so a host with cores to spare takes eight */
  return hw >= 32 ? 8u : (hw >= 8 ? 4u : (hw >= 4 ? 2u : 1u));
}

void staging_pool_main(StagingPool *p, unsigned index)
{
  unsigned seen = 0;
  for (;;) {
    std::function<void(unsigned)> job;
    {
      std::unique_lock<std::mutex> g(p->lock);
      p->work.wait(g, [&] { return p->stop || p->generation != seen; });
      if (p->stop) return;
      seen = p->generation;
      job = p->job;
    }
    job(index);
    {
      std::lock_guard<std::mutex> g(p->lock);
      if (--p->pending == 0) p->done.notify_one();
    }
  }
}

/* Run body(first, last) over [0, count) cut into contiguous ranges of about equal cost, one per thread
 * (the caller's included).  `prefix` has count + 1 entries: the running cost. */
template <class Body>
void staged_span(AADHipContext *ctx, uint32_t first, uint32_t count, const std::vector<uint64_t> &prefix, Body body)
{
  const uint64_t base = prefix[first];
  const unsigned want = count - first < 2 || prefix[count] - base < kParallelStagingAbove ? 1u : staging_threads(ctx);
  if (want <= 1) {
    body(first, count);
    return;
  }
  if (ctx->pool != nullptr && ctx->pool->threads.size() + 1 != want) staging_pool_stop(ctx);
  if (ctx->pool == nullptr) {
    ctx->pool = new (std::nothrow) StagingPool();
    if (ctx->pool == nullptr) {
      body(first, count);
      return;
    }
    /* These entry points are extern "C": an exception must not leave them.  A thread that cannot be created
     * (RLIMIT_NPROC, a cgroup's pids limit: std::system_error) ends the pool - the threads that did start are joined - and
     * the caller copies alone. */
    try {
      for (unsigned t = 1; t < want; t++) ctx->pool->threads.emplace_back(staging_pool_main, ctx->pool, t);
    } catch (...) {
      staging_pool_stop(ctx);
      body(first, count);
      return;
    }
  }
  StagingPool *p = ctx->pool;
  const unsigned parts = (unsigned)p->threads.size() + 1;
  auto bound = [&](unsigned t) -> uint32_t { /* first item of part t */
    if (t >= parts) return count;
    if (t == 0) return first;
    const uint64_t target = base + (prefix[count] - base) / parts * t;
    uint32_t lo = first, hi = count;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (prefix[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  auto part = [&](unsigned t) {
    const uint32_t a = bound(t), b = bound(t + 1);
    if (b > a) body(a, b);
  };
  {
    std::lock_guard<std::mutex> g(p->lock);
    p->job = part;
    p->pending = parts - 1;
    p->generation++;
  }
  p->work.notify_all();
  part(0);
  std::unique_lock<std::mutex> g(p->lock);
  p->done.wait(g, [&] { return p->pending == 0; });
}

bool ensure_events(AADHipContext *ctx)
{
  if (ctx->have_events) return true;
  if (!hip_ok(ctx, hipEventCreateWithFlags(&ctx->chunk_done[0], hipEventDisableTiming), "hipEventCreate")) return false;
  if (!hip_ok(ctx, hipEventCreateWithFlags(&ctx->chunk_done[1], hipEventDisableTiming), "hipEventCreate")) {
    (void)hipEventDestroy(ctx->chunk_done[0]);
    return false;
  }
  for (int i = 0; i < 3; i++)
    if (!hip_ok(ctx, hipEventCreateWithFlags(&ctx->piece_done[i], hipEventDisableTiming), "hipEventCreate")) {
      for (int k = 0; k < i; k++) (void)hipEventDestroy(ctx->piece_done[k]);
      (void)hipEventDestroy(ctx->chunk_done[0]);
      (void)hipEventDestroy(ctx->chunk_done[1]);
      return false;
    }
  ctx->have_events = true;
  return true;
}

/* the copy streams and their events: made at a context's first cut batch (a process that only ever
 * sends small calls keeps one stream - every extra one costs the runtime a little on each call) */
bool ensure_pipeline(AADHipContext *ctx)
{
  if (ctx->have_pipeline) return true;
  hipEvent_t ev[4];
  int made = 0;
  for (; made < 4; made++)
    if (!hip_ok(ctx, hipEventCreateWithFlags(&ev[made], hipEventDisableTiming), "hipEventCreate")) break;
  bool ok = made == 4;
  if (ok && !hip_ok(ctx, hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking), "hipStreamCreate")) ok = false;
  if (ok && !hip_ok(ctx, hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking), "hipStreamCreate")) {
    (void)hipStreamDestroy(ctx->up_stream);
    ok = false;
  }
  if (!ok) {
    for (int i = 0; i < made; i++) (void)hipEventDestroy(ev[i]);
    return false;
  }
  for (int b = 0; b < 2; b++) {
    ctx->uploaded[b] = ev[b];
    ctx->computed[b] = ev[2 + b];
  }
  ctx->have_pipeline = true;
  return true;
}

/* make `to` wait for what `from` holds so far */
bool hop(AADHipContext *ctx, hipEvent_t event, hipStream_t from, hipStream_t to)
{
  if (from == to) return true;
  return hip_ok(ctx, hipEventRecord(event, from), "hipEventRecord") &&
         hip_ok(ctx, hipStreamWaitEvent(to, event, 0), "hipStreamWaitEvent");
}

bool state_reserve(AADHipContext *ctx, size_t records)
{
  if (records <= ctx->state_capacity) return true;
  if (ctx->d_state) (void)hipFree(ctx->d_state); /* waits for the device: nothing is still reading it */
  ctx->d_state = nullptr;
  ctx->state_capacity = 0;
  const size_t want = records + records / 4 + 64;
  if (!hip_ok(ctx, hipMalloc(&ctx->d_state, sizeof(AADHipLaneState) * want), "hipMalloc lane states")) return false;
  ctx->state_capacity = want;
  return true;
}

/*
 * The tile pipeline of the host-memory calls.  Every tile the planner hands out (aad_tiles.h) goes through one of two pairs of
 * pinned blocks, alternately: fill and copy up (up), launch (run), copy down (down).  It is handed to the caller
 * when its pair comes round again, or at the end, older first - so the host fills tile k + 1 and drains tile k - 1 while tile k is
 * on the device.  Tile is aad::EncodeTile or aad::DecodeTile; the callables are all that differs between the two directions:
 *   prepare(step, order, &tile) -> AADApiResult  lay the tile out and make its launch arguments: no device work
 *   fill(tile, hin, first, last) -> bool          write rows [first, last) of the input block, with first == 0 also what lies before them
 *   launch(tile, din, dout, hout) -> bool         queue the kernel, and what else belongs on the compute stream (ctx->stream)
 *   deliver(tile, hout, first, last)              hand rows [first, last) of the output block to the caller
 * A batch that goes as one tile has its big copy - the input's where Tile::kCutUp, else the output's - cut into pieces.  On return
 * nothing of the call is in flight, whatever the result.
 */
template <class Tile, class Prepare, class Fill, class Launch, class Deliver>
AADApiResult run_tiles(AADHipContext *ctx, aad::TilePlanner &planner, bool piped, Prepare prepare, Fill fill, Launch launch, Deliver deliver)
{
  if (piped && !ensure_pipeline(ctx)) return AAD_APIRESULT_NG;
  /* the streams a tile's three stages run on: all the context's own for a batch that goes as one tile (no cross-stream hop on the
   * latency path of small calls), three different ones for a cut batch */
  const hipStream_t up = piped ? ctx->up_stream : ctx->stream, run = ctx->stream, down = piped ? ctx->down_stream : ctx->stream;
  struct Flight {
    bool active = false;
    Tile tile;
    uint32_t pieces = 1, piece_end[aad::kMaxPieces] = {}; /* row where each piece of the output copy ends */
  } flight[2];
  uint64_t sequence = 0;
  /* recorded behind piece p of pair b's output copy */
  auto down_event = [&](int b, uint32_t p, uint32_t pieces) { return p + 1 == pieces ? ctx->chunk_done[b] : ctx->piece_done[p]; };

  /* wait for the tile on pair b and hand it to the caller */
  auto finish = [&](int b) -> bool {
    Flight &f = flight[b];
    if (!f.active) return true;
    f.active = false;
    bool ok = true;
    for (uint32_t p = 0, first = 0; p < f.pieces; first = f.piece_end[p++]) {
      /* every piece is waited for, also after a failure: the buffers must be idle on return */
      if (!hip_ok(ctx, hipEventSynchronize(down_event(b, p, f.pieces)), "hipEventSynchronize")) ok = false;
      if (ok) deliver(f.tile, static_cast<const uint8_t *>(ctx->out[b].host), first, f.piece_end[p]);
    }
    return ok;
  };

  AADApiResult rc = AAD_APIRESULT_OK;
  for (aad::TileStep step; rc == AAD_APIRESULT_OK && planner.next(&step);) {
    const int b = (int)(sequence & 1);
    if (!finish(b)) { rc = AAD_APIRESULT_NG; break; }
    Flight &f = flight[b];
    Tile &t = f.tile;
    rc = prepare(step, planner.order, &t);
    if (rc != AAD_APIRESULT_OK) break;
    rc = AAD_APIRESULT_NG;
    if (!staging_reserve(ctx, ctx->in[b], t.in_bytes + 64) || !staging_reserve(ctx, ctx->out[b], t.out_bytes + 64)) break;
    uint8_t *hin = static_cast<uint8_t *>(ctx->in[b].host), *din = static_cast<uint8_t *>(ctx->in[b].dev);
    uint8_t *hout = static_cast<uint8_t *>(ctx->out[b].host), *dout = static_cast<uint8_t *>(ctx->out[b].dev);
    bool ok = true;
    uint32_t up_end[aad::kMaxPieces];
    const uint32_t up_pieces = aad::copy_pieces(t, true, piped, up_end);
    size_t sent = 0, got = 0;
    for (uint32_t p = 0, first = 0; ok && p < up_pieces; first = up_end[p++]) {
      const size_t upto = p + 1 == up_pieces ? t.in_bytes : t.payload_off + (size_t)t.fill_cost[up_end[p]];
      ok = fill(t, hin, first, up_end[p]) && hip_ok(ctx, hipMemcpyAsync(din + sent, hin + sent, upto - sent, hipMemcpyHostToDevice, up), "H2D block");
      sent = upto;
    }
    if (!ok || !hop(ctx, ctx->uploaded[b], up, run)) break;
    if (!launch(t, din, dout, hout) || !hop(ctx, ctx->computed[b], run, down)) break;
    f.pieces = aad::copy_pieces(t, false, piped, f.piece_end);
    /* piece_done[] is ONE set of events for both flights: only a batch that travels as a single tile (nothing in the other
     * flight) may cut its copy into pieces */
    if (piped && f.pieces != 1) {
      snprintf(ctx->last_error, sizeof(ctx->last_error), "internal: a piped decode tile was cut into %u copy pieces", f.pieces);
      break;
    }
    for (uint32_t p = 0; ok && p < f.pieces; p++) {
      const size_t upto = p + 1 == f.pieces ? t.down_bytes : (size_t)t.drain_cost[f.piece_end[p]];
      if (upto > got) ok = hip_ok(ctx, hipMemcpyAsync(hout + got, dout + got, upto - got, hipMemcpyDeviceToHost, down), "D2H block");
      got = upto;
      ok = ok && hip_ok(ctx, hipEventRecord(down_event(b, p, f.pieces), down), "hipEventRecord");
    }
    if (!ok) break;
    sequence++;
    f.active = true;
    rc = AAD_APIRESULT_OK;
  }
  /* drain what is still in flight, older first - the pair that would be reused next - also on failure: the buffers must be idle on return */
  for (int b : {(int)(sequence & 1), (int)(~sequence & 1)}) rc = finish(b) ? rc : AAD_APIRESULT_NG;
  if (rc != AAD_APIRESULT_OK) /* a tile that failed half way may have left copies queued */
    for (hipStream_t s : {up, run, down}) (void)hipStreamSynchronize(s);
  return rc;
}

/* What every host-memory encode entry checks before any device work: the parameter makes a valid header (*h; its num_samples is
 * left at the last stream's), and per stream - its image size in (*sizes)[i] - first that it is not empty (INVALID_FORMAT,
 * src/aad_encoder.c:157-159), then, where the entry takes capacities (data_capacity non-null), that its buffer holds the image
 * (INSUFFICIENT_BUFFER). */
AADApiResult host_encode_check(const struct AADEncodeParameter *parameter, uint32_t num_streams, const uint32_t *num_samples,
                               const uint64_t *data_capacity, AADHeaderInfo *h, std::vector<uint64_t> *sizes)
{
  if (AADFormat_ParameterToHeader(parameter, 1, AAD_HIP_MAX_NUM_CHANNELS, h) != AAD_APIRESULT_OK ||
      !AADFormat_HeaderFieldsValid(h, AAD_HIP_MAX_NUM_CHANNELS))
    return AAD_APIRESULT_INVALID_FORMAT;
  sizes->resize(num_streams);
  for (uint32_t i = 0; i < num_streams; i++) {
    if (num_samples[i] == 0) return AAD_APIRESULT_INVALID_FORMAT;
    h->num_samples = num_samples[i];
    (*sizes)[i] = AADFormat_EncodedSize(h);
    if (data_capacity != nullptr && data_capacity[i] < (*sizes)[i]) return AAD_APIRESULT_INSUFFICIENT_BUFFER;
  }
  return AAD_APIRESULT_OK;
}

/*
 * Encode num_streams host streams.  fill(i, frame0, frames, dst) writes that range of stream i's
 * interleaved int16 frames, drain(i, offset, src, size) receives bytes [offset, offset + size) of
 * its .aad image.  `state` as in AADHip_EncodeBatch.
 */
template <class Fill, class Drain>
AADApiResult encode_host(AADHipContext *ctx, const struct AADEncodeParameter *parameter, uint32_t num_streams,
                         const uint32_t *num_samples, const uint64_t *data_capacity, uint64_t *output_size,
                         struct AADHipLaneState *state, Fill fill, Drain drain)
{
  AADHeaderInfo h;
  std::vector<uint64_t> sizes, blocks(num_streams);
  const AADApiResult checked = host_encode_check(parameter, num_streams, num_samples, data_capacity, &h, &sizes);
  if (checked != AAD_APIRESULT_OK) return checked;
  const uint32_t ch = h.num_channels, spb = h.num_samples_per_block;
  uint64_t total = 0;
  for (uint32_t i = 0; i < num_streams; i++) {
    blocks[i] = ((uint64_t)num_samples[i] + spb - 1) / spb;
    total += (uint64_t)num_samples[i] * ch * sizeof(int16_t) + sizes[i];
  }
  DeviceGuard guard(ctx);
  if (!guard.ok || !ensure_events(ctx)) return AAD_APIRESULT_NG;

  aad::TilePlanner planner(blocks.data(), num_streams, (uint64_t)spb * ch * sizeof(int16_t) + h.block_size, aad::tile_budget(ctx->tile_bytes, total));
  aad::EncodeRun run; /* interleaved frames, a stream table, images only */
  const AADApiResult rc = run_tiles<aad::EncodeTile>(ctx, planner, aad::batch_is_cut(ctx->tile_bytes, total),
      [&](const aad::TileStep &step, const std::vector<uint32_t> &order, aad::EncodeTile *t) {
        aad::encode_tile_layout(step, order, num_samples, sizes.data(), blocks.data(), ch, spb, h.block_size, parameter->num_encode_trials > 0, state != nullptr, t);
        return encode_plan_init(parameter, step.alive, t->table.data(), &run.args, t->lead, true);
      },
      [&](const aad::EncodeTile &t, uint8_t *hin, uint32_t first, uint32_t last) {
        if (first == 0) {
          if (t.carry && !state_reserve(ctx, (size_t)t.group_size * ch)) return false;
          memcpy(hin, t.table.data(), sizeof(AADHipStreamDesc) * t.table.size());
          for (uint32_t k = 0; t.state_in && k < t.step.alive; k++)
            memcpy(hin + t.table_bytes + sizeof(AADHipLaneState) * (size_t)k * ch, state + (size_t)t.items[k].stream * ch, sizeof(AADHipLaneState) * ch);
        }
        staged_span(ctx, first, last, t.fill_cost, [&](uint32_t x, uint32_t y) {
          for (uint32_t k = x; k < y; k++)
            fill(t.items[k].stream, (uint32_t)t.fill_frame0, t.table[k].num_samples, reinterpret_cast<int16_t *>(hin + t.payload_off) + t.table[k].pcm_offset);
        });
        return true;
      },
      [&](const aad::EncodeTile &t, uint8_t *din, uint8_t *dout, uint8_t *hout) {
        aad::EncodeArgs &a = run.args;
        aad::LaneStateRecord *d_state = static_cast<aad::LaneStateRecord *>(ctx->d_state);
        a.streams = reinterpret_cast<const aad::StreamDesc *>(din);
        a.pcm = reinterpret_cast<const int16_t *>(din + t.payload_off);
        a.data = dout;
        a.state = t.state_in ? reinterpret_cast<const aad::LaneStateRecord *>(din + t.table_bytes) : (t.step.group_first ? nullptr : d_state);
        a.state_out = t.carry ? d_state : (t.state_back ? reinterpret_cast<aad::LaneStateRecord *>(dout + t.data_bytes) : nullptr);
        if (run_encode(ctx, run) != AAD_APIRESULT_OK) return false;
        /* from the device-side records on the compute stream: the next group's first launch overwrites them */
        return !(t.carry && t.state_back) ||
               hip_ok(ctx, hipMemcpyAsync(hout + t.data_bytes, d_state, t.out_bytes - t.data_bytes, hipMemcpyDeviceToHost, ctx->stream), "D2H lane states");
      },
      [&](const aad::EncodeTile &t, const uint8_t *out, uint32_t first, uint32_t last) { /* one piece: the whole tile */
        staged_span(ctx, first, last, t.drain_cost, [&](uint32_t lo, uint32_t hi) {
          for (uint32_t k = lo; k < hi; k++) {
            const aad::ImageSlice &d = t.items[k];
            drain(d.stream, d.dst, out + d.src, d.bytes);
            if (d.patch_count) { /* first tile of a longer stream: the header carries the whole count */
              const uint32_t all = num_samples[d.stream];
              const uint8_t be[4] = {(uint8_t)(all >> 24), (uint8_t)(all >> 16), (uint8_t)(all >> 8), (uint8_t)all};
              drain(d.stream, 14, be, 4);
            }
          }
        });
        const AADHipLaneState *records = reinterpret_cast<const AADHipLaneState *>(out + t.data_bytes);
        for (size_t slot = 0; slot < t.state_order.size(); slot++)
          memcpy(state + (size_t)t.state_order[slot] * ch, records + slot * ch, sizeof(AADHipLaneState) * ch);
      });
  if (rc == AAD_APIRESULT_OK && output_size) memcpy(output_size, sizes.data(), sizeof(uint64_t) * num_streams);
  return rc;
}

/* grow-only device block of a context (the device-resident waves of the segmented encode and of the reconstruction modes) */
bool device_block_reserve(AADHipContext *ctx, void **block, size_t *capacity, size_t bytes, const char *what)
{
  if (*capacity >= bytes) return true;
  if (*block) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(*block);
  }
  *block = nullptr;
  *capacity = 0;
  const size_t want = bytes + bytes / 8 + 4096; /* some slack, so that a slightly larger next wave does not reallocate */
  if (hipMalloc(block, want) == hipSuccess) {
    *capacity = want;
    return true;
  }
  (void)hipGetLastError();
  *block = nullptr;
  if (!hip_ok(ctx, hipMalloc(block, bytes), what)) {
    *block = nullptr;
    return false;
  }
  *capacity = bytes;
  return true;
}

/* bytes of the pinned chunks that stage a device-resident wave */
uint64_t staging_chunk(const AADHipContext *ctx) { return ctx->tile_bytes > 0 ? (uint64_t)ctx->tile_bytes : aad::kChunkBudget; }

/* The staging of a device-resident wave, on the context's own stream through its two pinned input / output blocks.
 * stage_up: bytes [0, bytes) of the device block d_dst in chunks; fill(lo, hi, host) writes bytes [lo, hi) to host[0 ..), and
 * chunk k is filled while chunk k - 1 is on the bus.  `what` names the copy in an error. */
template <class Fill>
bool stage_up(AADHipContext *ctx, uint8_t *d_dst, uint64_t bytes, size_t chunk, const char *what, Fill fill)
{
  const size_t stage = bytes < chunk ? (size_t)bytes + 64 : chunk;
  if (!staging_reserve(ctx, ctx->in[0], stage) || (bytes > chunk && !staging_reserve(ctx, ctx->in[1], stage))) return false;
  uint32_t k = 0;
  for (uint64_t lo = 0; lo < bytes; lo += chunk, k++) {
    const uint64_t hi = lo + chunk < bytes ? lo + chunk : bytes;
    /* the block's last copy, two rounds ago, has left it */
    if (k >= 2 && !hip_ok(ctx, hipEventSynchronize(ctx->chunk_done[k & 1]), "hipEventSynchronize")) return false;
    uint8_t *host = static_cast<uint8_t *>(ctx->in[k & 1].host);
    fill(lo, hi, host);
    if (!hip_ok(ctx, hipMemcpyAsync(d_dst + lo, host, (size_t)(hi - lo), hipMemcpyHostToDevice, ctx->stream), what) ||
        !hip_ok(ctx, hipEventRecord(ctx->chunk_done[k & 1], ctx->stream), "hipEventRecord"))
      return false;
  }
  return true;
}

/* stage_down: bytes [lo, hi) of the device block d_src in chunks; scatter(lo, hi, host) receives bytes [lo, hi) at host[0 ..), and
 * chunk k - 1 is scattered while chunk k is on the bus.  Nothing to bring down: no call is made. */
template <class Scatter>
bool stage_down(AADHipContext *ctx, const uint8_t *d_src, uint64_t lo, uint64_t hi, size_t chunk, Scatter scatter)
{
  if (hi <= lo) return true;
  const size_t stage = hi - lo < chunk ? (size_t)(hi - lo) + 64 : chunk;
  if (!staging_reserve(ctx, ctx->out[0], stage) || (hi - lo > chunk && !staging_reserve(ctx, ctx->out[1], stage))) return false;
  /* wait for chunk k's copy, queued one round before the one that is on the bus now, and hand it over */
  auto deliver = [&](uint32_t k, uint64_t c0, uint64_t c1) {
    if (!hip_ok(ctx, hipEventSynchronize(ctx->chunk_done[k & 1]), "hipEventSynchronize")) return false;
    scatter(c0, c1, static_cast<uint8_t *>(ctx->out[k & 1].host));
    return true;
  };
  uint32_t k = 0;
  for (uint64_t c0 = lo; c0 < hi; c0 += chunk, k++) {
    const uint64_t c1 = c0 + chunk < hi ? c0 + chunk : hi;
    if (!hip_ok(ctx, hipMemcpyAsync(ctx->out[k & 1].host, d_src + c0, (size_t)(c1 - c0), hipMemcpyDeviceToHost, ctx->stream), "D2H block") ||
        !hip_ok(ctx, hipEventRecord(ctx->chunk_done[k & 1], ctx->stream), "hipEventRecord"))
      return false;
    if (k > 0 && !deliver(k - 1, c0 - chunk, c0)) return false;
  }
  return deliver(k - 1, lo + (uint64_t)(k - 1) * chunk, hi);
}

/* device bytes a wave may take: what is free now plus what this context's own grow-only blocks already hold, less a quarter for
 * everybody else; a forced tile size forces small waves too (64 tiles' worth), so that the tests walk every path */
bool wave_budget(AADHipContext *ctx, uint64_t *budget)
{
  if (ctx->tile_bytes > 0) {
    *budget = (uint64_t)ctx->tile_bytes * 64u;
    return true;
  }
  DeviceGuard guard(ctx);
  size_t free_bytes = 0, total_bytes = 0;
  if (!guard.ok || !hip_ok(ctx, hipMemGetInfo(&free_bytes, &total_bytes), "hipMemGetInfo")) return false;
  const uint64_t own = ctx->rc_in_capacity + ctx->rc_out_capacity + ctx->scratch_capacity;
  *budget = ((uint64_t)free_bytes + own) / 4 * 3;
  return true;
}

/*
 * Segmented encode of host streams (AADHip_SegmentedEncodeBatch).  The serial path's tiles are block ranges of every stream of a
 * group with the predictor state carried between them; a segmented encode has no state to carry, and what it needs is all its
 * chains in ONE launch - a launch costs a chain's (L + W) blocks however few chains it holds.  So the COMPUTE is whole, as in
 * the reconstruction modes: a wave of consecutive chains (aad_segments.h build_segment_waves) is resident on the device - its chain
 * table and every chain's frames, warm-up included, then its output - and one kernel encodes all of it; only the STAGING is cut,
 * the input going up and the output coming down through the context's two pinned blocks in chunks, chunk k + 1 being filled /
 * chunk k - 1 being scattered while chunk k is on the bus.  A batch beyond three quarters of the device's free memory runs as
 * several waves.  No chain brings a look-back block: the trial search of a chain's first block has none, whatever precedes it in
 * the stream.  Each stream's file header, with the whole stream's count, is written by its first chain on the device.
 * fill(i, offset, size, dst): bytes [offset, offset + size) of stream i's interleaved int16 PCM; drain as in encode_host.
 */
template <class Fill, class Drain>
AADApiResult encode_host_segmented(AADHipContext *ctx, const struct AADEncodeParameter *parameter, const struct AADHipSegmentation *seg,
                                   uint32_t num_streams, const uint32_t *num_samples, const uint64_t *data_capacity,
                                   uint64_t *output_size, Fill fill, Drain drain)
{
  AADHeaderInfo h;
  std::vector<uint64_t> sizes;
  AADApiResult rc = host_encode_check(parameter, num_streams, num_samples, data_capacity, &h, &sizes);
  if (rc != AAD_APIRESULT_OK) return rc;
  const uint32_t ch = h.num_channels, spb = h.num_samples_per_block;
  aad::EncodeRun run; /* interleaved frames, each wave's chain table (use_chain_table), images only */
  rc = encode_plan_init(parameter, 0, nullptr, &run.args);
  if (rc != AAD_APIRESULT_OK) return rc;
  uint64_t budget;
  if (!wave_budget(ctx, &budget)) return AAD_APIRESULT_NG;
  std::vector<aad::SegmentWave> waves;
  if (!aad::build_segment_waves(num_samples, sizes.data(), num_streams, ch, spb, h.block_size, seg->segment_blocks,
                                seg->warmup_blocks, budget, &waves)) {
    snprintf(ctx->last_error, sizeof(ctx->last_error), "segmented encode: more than %u chains", (unsigned)UINT32_MAX);
    return AAD_APIRESULT_INVALID_ARGUMENT;
  }
  DeviceGuard guard(ctx);
  if (!guard.ok || !ensure_events(ctx)) return AAD_APIRESULT_NG;
  const size_t chunk = (size_t)round_up(staging_chunk(ctx) < 4096 ? 4096 : staging_chunk(ctx), 64);
  std::vector<uint64_t> row, spot; /* per chain of a wave: where its PCM starts in the input block, its bytes in the output block */
  for (size_t wi = 0; wi < waves.size() && rc == AAD_APIRESULT_OK; wi++) {
    const aad::SegmentWave &t = waves[wi];
    const uint32_t n = (uint32_t)t.chains.size();
    /* input block: chain table | pcm ; output block: lead-in | the chains' bytes */
    const uint64_t table_bytes = round_up(sizeof(aad::ChainDesc) * (uint64_t)n, 64), in_bytes = table_bytes + t.pcm_elems * sizeof(int16_t);
    row.resize((size_t)n + 1);
    spot.resize((size_t)n + 1);
    for (uint32_t k = 0; k < n; k++) {
      row[k] = table_bytes + t.chains[k].pcm_offset * sizeof(int16_t);
      spot[k] = t.where[k].out_offset;
    }
    row[n] = in_bytes;
    spot[n] = t.out_bytes;
    rc = AAD_APIRESULT_NG;
    if (!device_block_reserve(ctx, &ctx->d_rc_in, &ctx->rc_in_capacity, in_bytes + 64, "hipMalloc segmented encode input") ||
        !device_block_reserve(ctx, &ctx->d_rc_out, &ctx->rc_out_capacity, t.out_bytes + 64, "hipMalloc segmented encode output"))
      break;
    uint8_t *d_in = static_cast<uint8_t *>(ctx->d_rc_in), *d_out = static_cast<uint8_t *>(ctx->d_rc_out);

    /* ---- up: the input block, the table's bytes and every chain's frames as they fall into a chunk ---- */
    const bool up = stage_up(ctx, d_in, in_bytes, chunk, "H2D block", [&](uint64_t lo, uint64_t hi, uint8_t *host) {
      const uint64_t table_end = sizeof(aad::ChainDesc) * (uint64_t)n;
      if (lo < table_end)
        memcpy(host, reinterpret_cast<const uint8_t *>(t.chains.data()) + lo, (size_t)((hi < table_end ? hi : table_end) - lo));
      uint32_t a, b;
      aad::row_span(row, lo, hi, &a, &b);
      staged_span(ctx, a, b, row, [&](uint32_t x, uint32_t y) {
        for (uint32_t c = x; c < y; c++) {
          const uint64_t r0 = row[c], r1 = r0 + (uint64_t)t.chains[c].num_frames * ch * sizeof(int16_t);
          const uint64_t c0 = r0 > lo ? r0 : lo, c1 = r1 < hi ? r1 : hi;
          if (c1 > c0)
            fill(t.where[c].stream, (uint64_t)t.where[c].frame0 * ch * sizeof(int16_t) + (c0 - r0), c1 - c0, host + (c0 - lo));
        }
      });
    });
    if (!up) break;

    /* ---- compute: one launch over every chain of the wave ---- */
    use_chain_table(&run, reinterpret_cast<const aad::ChainDesc *>(d_in), n);
    run.args.pcm = reinterpret_cast<const int16_t *>(d_in + table_bytes);
    run.args.data = d_out;
    if (run_encode(ctx, run) != AAD_APIRESULT_OK) break;

    /* ---- down: bytes [out_begin, out_bytes) of the output block, each chain's to its place in its stream's image ---- */
    const bool down = stage_down(ctx, d_out, t.out_begin, t.out_bytes, chunk, [&](uint64_t lo, uint64_t hi, const uint8_t *host) {
      uint32_t a, b;
      aad::row_span(spot, lo, hi, &a, &b);
      staged_span(ctx, a, b, spot, [&](uint32_t x, uint32_t y) {
        for (uint32_t c = x; c < y; c++) {
          const aad::WaveChain &w = t.where[c];
          const uint64_t c0 = w.out_offset > lo ? w.out_offset : lo, e = w.out_offset + w.image_bytes, c1 = e < hi ? e : hi;
          if (c1 > c0) drain(w.stream, w.image_offset + (c0 - w.out_offset), host + (c0 - lo), c1 - c0);
        }
      });
    });
    if (!down) break;
    rc = AAD_APIRESULT_OK;
  }
  if (rc != AAD_APIRESULT_OK) (void)hipStreamSynchronize(ctx->stream); /* nothing of this call stays in flight */
  if (rc == AAD_APIRESULT_OK && output_size) memcpy(output_size, sizes.data(), sizeof(uint64_t) * num_streams);
  return rc;
}

/*
 * Decode num_streams host images of one format.  fill(i, offset, size, dst) writes bytes
 * [offset, offset + size) of stream i's image, drain(i, frame0, src, frames) receives that range
 * of its interleaved int16 frames.  Tiles carry bare blocks (the file header stays on the host).
 */
template <class Fill, class Drain>
AADApiResult decode_host(AADHipContext *ctx, const struct AADHeaderInfo *format, int32_t has_file_header,
                         uint32_t num_streams, const uint64_t *data_size, const uint32_t *num_samples,
                         uint32_t *decoded_frames, Fill fill, Drain drain)
{
  const uint32_t ch = format->num_channels, head = has_file_header ? AAD_HEADER_SIZE : 0;
  const uint32_t spb = format->num_samples_per_block, bs = format->block_size;
  if (ch == 0 || bs == 0 || spb == 0) return AAD_APIRESULT_INVALID_FORMAT;
  std::vector<AADHipStreamDesc> table(num_streams);
  std::vector<uint64_t> prefix((size_t)num_streams + 1), blocks(num_streams);
  uint64_t total = 0;
  for (uint32_t i = 0; i < num_streams; i++) {
    table[i] = {0, 0, data_size[i], num_samples[i], 0};
    total += data_size[i] + (uint64_t)num_samples[i] * ch * sizeof(int16_t);
  }
  {
    /* the whole batch is validated before the first tile runs: a bad stream fails the call with
     * nothing decoded, as it did when a batch was one launch */
    aad::DecodeArgs whole;
    const AADApiResult ok = decode_plan_init(format, has_file_header, num_streams, table.data(), prefix.data(), &whole);
    if (ok != AAD_APIRESULT_OK) return ok;
    for (uint32_t i = 0; i < num_streams; i++) blocks[i] = prefix[i + 1] - prefix[i];
  }
  DeviceGuard guard(ctx);
  if (!guard.ok || !ensure_events(ctx)) return AAD_APIRESULT_NG;
  if (decoded_frames) memset(decoded_frames, 0, sizeof(uint32_t) * num_streams);

  uint64_t block_cost;
  const uint64_t overreach = aad::decode_overreach(ch, format->bits_per_sample, spb, bs, &block_cost);
  aad::TilePlanner planner(blocks.data(), num_streams, block_cost, aad::tile_budget(ctx->tile_bytes, total));
  aad::DecodeArgs a;
  return run_tiles<aad::DecodeTile>(ctx, planner, aad::batch_is_cut(ctx->tile_bytes, total),
      [&](const aad::TileStep &step, const std::vector<uint32_t> &order, aad::DecodeTile *t) {
        aad::decode_tile_layout(step, order, data_size, num_samples, blocks.data(), ch, spb, bs, head, overreach, t);
        prefix.resize((size_t)step.alive + 1);
        return decode_plan_init(format, 0, step.alive, t->table.data(), prefix.data(), &a, t->tile_blocks.data());
      },
      [&](const aad::DecodeTile &t, uint8_t *hin, uint32_t first, uint32_t last) { /* one piece: the whole tile */
        memcpy(hin, t.table.data(), sizeof(AADHipStreamDesc) * t.table.size());
        memcpy(hin + t.table_bytes, prefix.data(), sizeof(uint64_t) * prefix.size());
        staged_span(ctx, first, last, t.fill_cost, [&](uint32_t lo, uint32_t hi) {
          for (uint32_t k = lo; k < hi; k++)
            fill(t.items[k].stream, t.fill_byte0, t.table[k].data_size, hin + t.payload_off + t.table[k].data_offset);
        });
        return true;
      },
      [&](const aad::DecodeTile &t, uint8_t *din, uint8_t *dout, uint8_t *) {
        a.streams = reinterpret_cast<const aad::StreamDesc *>(din);
        a.block_prefix = reinterpret_cast<const uint64_t *>(din + t.table_bytes);
        a.data = din + t.payload_off;
        a.pcm = reinterpret_cast<int16_t *>(dout);
        if ((reinterpret_cast<uintptr_t>(a.pcm) & 63u) != 0) a.stream_stores = 0;
        return run_decode(ctx, a) == AAD_APIRESULT_OK;
      },
      [&](const aad::DecodeTile &t, const uint8_t *out, uint32_t first, uint32_t last) {
        staged_span(ctx, first, last, t.drain_cost, [&](uint32_t lo, uint32_t hi) {
          for (uint32_t k = lo; k < hi; k++) {
            const aad::FrameRun &d = t.items[k];
            if (d.frames) drain(d.stream, (uint32_t)d.frame0, reinterpret_cast<const int16_t *>(out) + d.src, (uint32_t)d.frames);
            if (decoded_frames) decoded_frames[d.stream] += (uint32_t)d.frames; /* one item per stream and tile */
          }
        });
      });
}

} /* namespace */

extern "C" {

AADApiResult AADHip_EncodeBatch(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                uint32_t num_streams, const int16_t *const *pcm, const uint32_t *num_samples,
                                uint8_t *const *data, const uint64_t *data_capacity, uint64_t *output_size,
                                struct AADHipLaneState *state)
{
  if (ctx == nullptr || parameter == nullptr || (num_streams != 0 && (pcm == nullptr || num_samples == nullptr ||
      data == nullptr || data_capacity == nullptr)))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  if (num_streams == 0) return AAD_APIRESULT_OK;
  for (uint32_t i = 0; i < num_streams; i++)
    if (pcm[i] == nullptr || data[i] == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  const size_t frame_bytes = sizeof(int16_t) * parameter->num_channels;
  return encode_host(ctx, parameter, num_streams, num_samples, data_capacity, output_size, state,
                     [&](uint32_t i, uint32_t frame0, uint32_t frames, int16_t *dst) {
                       memcpy(dst, pcm[i] + (size_t)frame0 * parameter->num_channels, (size_t)frames * frame_bytes);
                     },
                     [&](uint32_t i, uint64_t offset, const uint8_t *src, uint64_t size) { memcpy(data[i] + offset, src, size); });
}

AADApiResult AADHip_SegmentedEncodeBatch(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                         const struct AADHipSegmentation *segmentation, uint32_t num_streams,
                                         const int16_t *const *pcm, const uint32_t *num_samples, uint8_t *const *data,
                                         const uint64_t *data_capacity, uint64_t *output_size)
{
  if (ctx == nullptr || parameter == nullptr || segmentation == nullptr || segmentation->segment_blocks == 0 ||
      (num_streams != 0 && (pcm == nullptr || num_samples == nullptr || data == nullptr || data_capacity == nullptr)))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  if (num_streams == 0) return AAD_APIRESULT_OK;
  for (uint32_t i = 0; i < num_streams; i++)
    if (pcm[i] == nullptr || data[i] == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
  return encode_host_segmented(ctx, parameter, segmentation, num_streams, num_samples, data_capacity, output_size,
                               [&](uint32_t i, uint64_t offset, uint64_t size, uint8_t *dst) {
                                 memcpy(dst, reinterpret_cast<const uint8_t *>(pcm[i]) + offset, (size_t)size);
                               },
                               [&](uint32_t i, uint64_t offset, const uint8_t *src, uint64_t size) { memcpy(data[i] + offset, src, size); });
}

/* AADEncoder_EncodeWhole's data path (src/aad_encoder.c:814-891): planar int32 rows in, one image
 * out.  The planar -> interleaved int16 conversion writes straight into the pinned block; samples
 * must already be in int16 range, which the reference only asserts (src/aad_encoder.c:612) -
 * out-of-range input saturates. */
AADApiResult AADHipInternal_EncodePlanar32(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                           const int32_t *const *input, uint32_t num_samples, uint8_t *data,
                                           uint64_t data_capacity, uint64_t *output_size, struct AADHipLaneState *state)
{
  const uint32_t ch = parameter->num_channels;
  return encode_host(ctx, parameter, 1, &num_samples, &data_capacity, output_size, state,
                     [&](uint32_t, uint32_t frame0, uint32_t frames, int16_t *dst) {
                       for (uint32_t c = 0; c < ch; c++) {
                         const int32_t *x = input[c] + frame0;
                         int16_t *d = dst + c;
                         for (uint32_t s = 0; s < frames; s++, d += ch) {
                           const int32_t v = x[s];
                           *d = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
                         }
                       }
                     },
                     [&](uint32_t, uint64_t offset, const uint8_t *src, uint64_t size) { memcpy(data + offset, src, size); });
}

/* shared by AADHip_DecodeBatch (file images) and the legacy AADDecoder_DecodeBlock (bare block) */
AADApiResult AADHipInternal_DecodeHost(struct AADHipContext *ctx, const struct AADHeaderInfo *format,
                                       int32_t has_file_header, uint32_t num_streams,
                                       const uint8_t *const *data, const uint64_t *data_size,
                                       const uint32_t *num_samples, int16_t *const *pcm, uint32_t *decoded_frames)
{
  const size_t frame_bytes = sizeof(int16_t) * format->num_channels;
  return decode_host(ctx, format, has_file_header, num_streams, data_size, num_samples, decoded_frames,
                     [&](uint32_t i, uint64_t offset, uint64_t size, uint8_t *dst) { memcpy(dst, data[i] + offset, size); },
                     [&](uint32_t i, uint32_t frame0, const int16_t *src, uint32_t frames) {
                       memcpy(pcm[i] + (size_t)frame0 * format->num_channels, src, (size_t)frames * frame_bytes);
                     });
}

/* AADDecoder_DecodeWhole / DecodeBlock's data path: one image (or bare block) in, planar int32
 * rows out, widened straight from the pinned block (src/aad_decoder.c:478-538, :321-475) */
AADApiResult AADHipInternal_DecodePlanar32(struct AADHipContext *ctx, const struct AADHeaderInfo *format,
                                           int32_t has_file_header, const uint8_t *data, uint64_t data_size,
                                           uint32_t want_frames, int32_t *const *buffer, uint32_t *decoded_frames)
{
  const uint32_t ch = format->num_channels;
  return decode_host(ctx, format, has_file_header, 1, &data_size, &want_frames, decoded_frames,
                     [&](uint32_t, uint64_t offset, uint64_t size, uint8_t *dst) { memcpy(dst, data + offset, size); },
                     [&](uint32_t, uint32_t frame0, const int16_t *src, uint32_t frames) {
                       for (uint32_t c = 0; c < ch; c++) {
                         int32_t *y = buffer[c] + frame0;
                         const int16_t *s = src + c;
                         for (uint32_t k = 0; k < frames; k++, s += ch) y[k] = *s;
                       }
                     });
}

AADApiResult AADHip_DecodeBatch(struct AADHipContext *ctx, uint32_t num_streams, const uint8_t *const *data,
                                const uint64_t *data_size, int16_t *const *pcm, const uint32_t *pcm_capacity_frames,
                                uint32_t *decoded_frames)
{
  if (ctx == nullptr || (num_streams != 0 && (data == nullptr || data_size == nullptr || pcm == nullptr ||
      pcm_capacity_frames == nullptr)))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  if (num_streams == 0) return AAD_APIRESULT_OK;
  std::vector<uint32_t> frames(num_streams);
  AADHeaderInfo format;
  for (uint32_t i = 0; i < num_streams; i++) {
    AADHeaderInfo h;
    if (data[i] == nullptr || pcm[i] == nullptr) return AAD_APIRESULT_INVALID_ARGUMENT;
    if (data_size[i] < AAD_HEADER_SIZE) return AAD_APIRESULT_INSUFFICIENT_DATA;
    if (!AADFormat_GetHeader(data[i], &h)) return AAD_APIRESULT_INVALID_FORMAT;
    if (!AADFormat_HeaderAcceptedByDecoder(&h, AAD_HIP_MAX_NUM_CHANNELS)) return AAD_APIRESULT_INVALID_FORMAT;
    if (i == 0) {
      format = h;
    } else if (h.num_channels != format.num_channels || h.bits_per_sample != format.bits_per_sample ||
               h.block_size != format.block_size || h.num_samples_per_block != format.num_samples_per_block ||
               h.ch_process_method != format.ch_process_method) {
      return AAD_APIRESULT_INVALID_FORMAT; /* one format per batch */
    }
    if (pcm_capacity_frames[i] < h.num_samples) return AAD_APIRESULT_INSUFFICIENT_BUFFER;
    frames[i] = h.num_samples;
  }
  return AADHipInternal_DecodeHost(ctx, &format, 1, num_streams, data, data_size, frames.data(), pcm, decoded_frames);
}

/* ------------------------------------------------------------------- reconstruction modes -- */

/* segmentation: null for the reference encoder's images, else those of a segmented encode plan */
static AADApiResult reconstruct_plan_create(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                            const struct AADHipSegmentation *segmentation, uint32_t num_streams,
                                            const struct AADHipStreamDesc *streams, struct AADHipReconstructPlan **plan)
{
  *plan = nullptr;
  AADHipReconstructPlan *p = new (std::nothrow) AADHipReconstructPlan();
  if (p == nullptr) return AAD_APIRESULT_NG;
  memset(static_cast<void *>(p), 0, sizeof(*p));
  p->ctx = ctx;
  AADApiResult rc = encode_plan_create(ctx, parameter, nullptr, nullptr, segmentation, num_streams, streams, &p->encode);
  if (rc == AAD_APIRESULT_OK) {
    /* the decoder sees exactly the images the encoder writes */
    AADHeaderInfo h;
    std::vector<AADHipStreamDesc> images(streams, streams + num_streams);
    std::vector<uint64_t> prefix((size_t)num_streams + 1);
    uint64_t segments = 0;
    (void)AADFormat_ParameterToHeader(parameter, 1, AAD_HIP_MAX_NUM_CHANNELS, &h);
    for (uint32_t i = 0; i < num_streams; i++) {
      h.num_samples = streams[i].num_samples;
      images[i].data_size = AADFormat_EncodedSize(&h);
      prefix[i] = segments;
      segments += ((uint64_t)streams[i].num_samples * h.num_channels + aad::kCompareSegment - 1) / aad::kCompareSegment;
    }
    prefix[num_streams] = segments;
    rc = AADHip_DecodePlanCreate(ctx, &h, 1, num_streams, images.data(), &p->decode);
    if (rc == AAD_APIRESULT_OK) {
      DeviceGuard guard(ctx);
      if (!guard.ok || !upload(ctx, &p->d_segment_prefix, prefix.data(), prefix.size()) ||
          !hip_ok(ctx, hipMalloc((void **)&p->d_partials, sizeof(aad::ErrorPartial) * (segments ? segments : 1)), "hipMalloc partials"))
        rc = AAD_APIRESULT_NG;
    }
    p->args.streams = p->decode ? p->decode->d_streams : nullptr;
    p->args.segment_prefix = p->d_segment_prefix;
    p->args.total_segments = segments;
    p->args.num_streams = num_streams;
    p->args.channels = h.num_channels;
  }
  if (rc != AAD_APIRESULT_OK) {
    AADHip_ReconstructPlanDestroy(p);
    return rc;
  }
  *plan = p;
  return AAD_APIRESULT_OK;
}

AADApiResult AADHip_ReconstructPlanCreate(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                          uint32_t num_streams, const struct AADHipStreamDesc *streams,
                                          struct AADHipReconstructPlan **plan)
{
  if (ctx == nullptr || parameter == nullptr || plan == nullptr || (num_streams != 0 && streams == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  return reconstruct_plan_create(ctx, parameter, nullptr, num_streams, streams, plan);
}

AADApiResult AADHip_SegmentedReconstructPlanCreate(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                                   const struct AADHipSegmentation *segmentation, uint32_t num_streams,
                                                   const struct AADHipStreamDesc *streams, struct AADHipReconstructPlan **plan)
{
  if (ctx == nullptr || parameter == nullptr || segmentation == nullptr || plan == nullptr || (num_streams != 0 && streams == nullptr))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  *plan = nullptr;
  if (segmentation->segment_blocks == 0) return AAD_APIRESULT_INVALID_ARGUMENT;
  return reconstruct_plan_create(ctx, parameter, segmentation, num_streams, streams, plan);
}

void AADHip_ReconstructPlanDestroy(struct AADHipReconstructPlan *plan)
{
  if (plan == nullptr) return;
  AADHip_EncodePlanDestroy(plan->encode); /* each synchronises the stream first */
  AADHip_DecodePlanDestroy(plan->decode);
  {
    DeviceGuard guard(plan->ctx);
    if (guard.ok) {
      (void)hipStreamSynchronize(plan->ctx->stream);
      if (plan->d_segment_prefix) (void)hipFree(plan->d_segment_prefix);
      if (plan->d_partials) (void)hipFree(plan->d_partials);
    }
  }
  delete plan;
}

AADApiResult AADHip_ReconstructPlanRun(struct AADHipReconstructPlan *plan, const int16_t *device_pcm, uint8_t *device_data,
                                       int16_t *device_out, int32_t output_kind, struct AADHipErrorStats *device_stats)
{
  if (plan == nullptr || device_pcm == nullptr || device_data == nullptr || device_out == nullptr ||
      device_out == device_pcm)
    return AAD_APIRESULT_INVALID_ARGUMENT;
  if (output_kind != AAD_HIP_RECONSTRUCT_DECODED && output_kind != AAD_HIP_RECONSTRUCT_RESIDUAL)
    return AAD_APIRESULT_INVALID_ARGUMENT;
  AADHipContext *ctx = plan->ctx;
  /* a reconstruction is several kernels: pending AADHip_ContextSignalNextRun events are recorded in front of the first and
   * behind the last of them */
  const aad::LaunchSignal signal = take_signal(ctx);
  if (signal.start != nullptr && !hip_ok(ctx, hipEventRecord(signal.start, ctx->stream), "hipEventRecord")) return AAD_APIRESULT_NG;
  auto done = [&](AADApiResult r) -> AADApiResult {
    if (r == AAD_APIRESULT_OK && signal.stop != nullptr && !hip_ok(ctx, hipEventRecord(signal.stop, ctx->stream), "hipEventRecord")) return AAD_APIRESULT_NG;
    return r;
  };
  if (plan->args.num_streams == 0) return done(AAD_APIRESULT_OK);
  AADApiResult rc = AADHip_EncodePlanRun(plan->encode, device_pcm, device_data, nullptr);
  if (rc != AAD_APIRESULT_OK) return rc;
  rc = AADHip_DecodePlanRun(plan->decode, device_data, device_out);
  if (rc != AAD_APIRESULT_OK) return rc;
  if (device_stats == nullptr && output_kind == AAD_HIP_RECONSTRUCT_DECODED) return done(AAD_APIRESULT_OK);
  DeviceGuard guard(ctx);
  if (!guard.ok) return AAD_APIRESULT_NG;
  aad::CompareArgs a = plan->args;
  a.original = device_pcm;
  a.decoded = device_out;
  a.partials = device_stats ? plan->d_partials : nullptr;
  a.stats = reinterpret_cast<aad::ErrorStatsRecord *>(device_stats);
  a.write_residual = output_kind == AAD_HIP_RECONSTRUCT_RESIDUAL;
  a.sequential = ctx->compare_sequential ? 1u : 0u;
  if (a.total_segments > 0x7FFFFFFFull) return AAD_APIRESULT_INVALID_ARGUMENT;
  hipLaunchKernelGGL(aad::compare_segments_kernel, dim3((unsigned)a.total_segments), dim3(aad::kCompareThreads), 0, ctx->stream, a);
  if (device_stats)
    hipLaunchKernelGGL(aad::compare_finish_kernel, dim3(a.num_streams), dim3(64), 0, ctx->stream, a);
  return done(hip_ok(ctx, hipGetLastError(), "compare launch") ? AAD_APIRESULT_OK : AAD_APIRESULT_NG);
}

/*
 * Host-memory reconstruction.  The COMPUTE stays whole - every stream of a wave is encoded, decoded and compared by one
 * AADHip_ReconstructPlanRun over device-resident buffers, so that the encoder's block chains of all streams run side by side and
 * the statistics are summed per stream in the reference's order whatever the batch size - and only the STAGING is cut: the PCM goes
 * up and the output comes down through the context's two pinned blocks in chunks (the tile budget of the other host-memory entry
 * points: 16 MiB, or AAD_HIP_OPTION_TILE_KBYTES), chunk k + 1 being filled / chunk k - 1 being scattered by the host while chunk
 * k is on the bus.  Pinned memory is bounded by the chunk size; device memory holds 2 x PCM + images of a WAVE of whole streams,
 * and a batch that does not fit the device's free memory (288 GB on MI355X: ~60 G channel-samples) goes as several waves of
 * consecutive streams.  A forced tile size also forces small waves (64 tiles' worth), so that the tests walk every path.
 */
namespace {

struct ReconstructWave {
  uint32_t first, count;
};

/* device bytes a stream occupies in a wave: PCM in + PCM out (rows padded to 16 bytes), its image (padded to 16), its statistics */
uint64_t reconstruct_footprint(uint64_t samples, uint32_t ch, uint64_t image)
{
  return 2 * round_up(samples * ch, 8) * sizeof(int16_t) + round_up(image, 16) + sizeof(AADHipErrorStats);
}


/* one wave: streams [first, first + count) of the batch, device-resident compute, chunked staging */
AADApiResult reconstruct_wave(AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                              const struct AADHipSegmentation *segmentation, uint32_t count, const int16_t *const *pcm, const uint32_t *num_samples, int32_t output_kind,
                              int16_t *const *out_pcm, struct AADHipErrorStats *stats, uint64_t chunk_bytes)
{
  const uint32_t ch = parameter->num_channels;
  std::vector<AADHipStreamDesc> table(count);
  std::vector<uint64_t> byte_prefix((size_t)count + 1); /* start of every stream's row in the flat PCM block, in bytes */
  uint64_t pcm_elems = 0, data_bytes = 0;
  for (uint32_t i = 0; i < count; i++) {
    const uint64_t size = AADHip_CalculateEncodedSize(parameter, num_samples[i]);
    table[i].pcm_offset = pcm_elems;
    table[i].data_offset = data_bytes;
    table[i].data_size = size;
    table[i].num_samples = num_samples[i];
    table[i].reserved = 0;
    byte_prefix[i] = pcm_elems * sizeof(int16_t);
    pcm_elems += round_up((uint64_t)num_samples[i] * ch, 8);
    data_bytes += round_up(size, 16);
  }
  byte_prefix[count] = pcm_elems * sizeof(int16_t);
  AADHipReconstructPlan *plan = nullptr;
  AADApiResult rc = reconstruct_plan_create(ctx, parameter, segmentation, count, table.data(), &plan);
  if (rc != AAD_APIRESULT_OK) return rc;
  DeviceGuard guard(ctx);
  /* device: [pcm in] ; [pcm out | statistics] ; [images].  The statistics sit behind the output PCM so that one flat range
   * comes down. */
  const size_t pcm_bytes = pcm_elems * sizeof(int16_t), stats_bytes = stats ? sizeof(AADHipErrorStats) * (size_t)count : 0;
  const size_t stats_off = round_up(pcm_bytes, 64), out_bytes = stats_off + stats_bytes;
  const size_t chunk = (size_t)round_up(chunk_bytes < 4096 ? 4096 : chunk_bytes, 64);
  rc = AAD_APIRESULT_NG;
  do {
    if (!guard.ok || !ensure_events(ctx)) break;
    if (!device_block_reserve(ctx, &ctx->d_rc_in, &ctx->rc_in_capacity, pcm_bytes + 64, "hipMalloc reconstruction input") ||
        !device_block_reserve(ctx, &ctx->d_rc_out, &ctx->rc_out_capacity, out_bytes + 64, "hipMalloc reconstruction output") ||
        !device_block_reserve(ctx, &ctx->d_scratch, &ctx->scratch_capacity, data_bytes + 64, "hipMalloc image scratch"))
      break;
    uint8_t *d_in = static_cast<uint8_t *>(ctx->d_rc_in), *d_out = static_cast<uint8_t *>(ctx->d_rc_out);

    /* the rows of the streams that fall into bytes [lo, hi) of the flat PCM block <-> host block `base` (which holds byte lo at 0) */
    auto rows = [&](uint64_t lo, uint64_t hi, uint8_t *base, bool up) {
      uint32_t a, b;
      aad::row_span(byte_prefix, lo, hi, &a, &b);
      staged_span(ctx, a, b, byte_prefix, [&](uint32_t x, uint32_t y) {
        for (uint32_t i = x; i < y; i++) {
          const uint64_t r0 = byte_prefix[i], r1 = r0 + (uint64_t)num_samples[i] * ch * sizeof(int16_t);
          const uint64_t c0 = r0 > lo ? r0 : lo, c1 = r1 < hi ? r1 : hi;
          if (c1 <= c0) continue;
          if (up) memcpy(base + (c0 - lo), reinterpret_cast<const uint8_t *>(pcm[i]) + (c0 - r0), (size_t)(c1 - c0));
          else memcpy(reinterpret_cast<uint8_t *>(out_pcm[i]) + (c0 - r0), base + (c0 - lo), (size_t)(c1 - c0));
        }
      });
    };

    /* ---- up: the flat PCM block ---- */
    if (!stage_up(ctx, d_in, pcm_bytes, chunk, "H2D pcm", [&](uint64_t lo, uint64_t hi, uint8_t *host) { rows(lo, hi, host, true); })) break;

    /* ---- compute: one run over the whole wave ---- */
    rc = AADHip_ReconstructPlanRun(plan, reinterpret_cast<const int16_t *>(d_in), static_cast<uint8_t *>(ctx->d_scratch),
                                   reinterpret_cast<int16_t *>(d_out), output_kind,
                                   stats ? reinterpret_cast<AADHipErrorStats *>(d_out + stats_off) : nullptr);
    if (rc != AAD_APIRESULT_OK) break;
    rc = AAD_APIRESULT_NG;

    /* ---- down: [PCM (if wanted) | statistics] as one flat range.  Statistics only: nothing but 24 bytes per stream comes back. ---- */
    const uint64_t down_lo = out_pcm ? 0 : stats_off, down_hi = stats ? out_bytes : (out_pcm ? pcm_bytes : down_lo);
    const bool down = stage_down(ctx, d_out, down_lo, down_hi, chunk, [&](uint64_t lo, uint64_t hi, uint8_t *host) {
      if (out_pcm && lo < pcm_bytes) rows(lo, hi < pcm_bytes ? hi : pcm_bytes, host, false);
      if (stats && hi > stats_off) {
        const uint64_t s0 = lo > stats_off ? lo : stats_off;
        memcpy(reinterpret_cast<uint8_t *>(stats) + (s0 - stats_off), host + (s0 - lo), (size_t)(hi - s0));
      }
    });
    if (!down) break;
    if (!hip_ok(ctx, hipStreamSynchronize(ctx->stream), "sync")) break;
    rc = AAD_APIRESULT_OK;
  } while (0);
  if (rc != AAD_APIRESULT_OK) (void)hipStreamSynchronize(ctx->stream); /* nothing of this call stays in flight */
  AADHip_ReconstructPlanDestroy(plan);
  return rc;
}

/* AADHip_ReconstructBatch and its segmented form (segmentation non-null, segment_blocks checked) */
AADApiResult reconstruct_batch(AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                               const struct AADHipSegmentation *segmentation, uint32_t num_streams, const int16_t *const *pcm,
                               const uint32_t *num_samples, int32_t output_kind, int16_t *const *out_pcm, struct AADHipErrorStats *stats)
{
  if (num_streams == 0) return AAD_APIRESULT_OK;
  for (uint32_t i = 0; i < num_streams; i++)
    if (pcm[i] == nullptr || (out_pcm != nullptr && out_pcm[i] == nullptr)) return AAD_APIRESULT_INVALID_ARGUMENT;
  AADHeaderInfo h; /* the whole batch is validated before the first wave runs */
  std::vector<uint64_t> sizes, footprint(num_streams);
  const AADApiResult checked = host_encode_check(parameter, num_streams, num_samples, nullptr, &h, &sizes);
  if (checked != AAD_APIRESULT_OK) return checked;
  for (uint32_t i = 0; i < num_streams; i++) footprint[i] = reconstruct_footprint(num_samples[i], h.num_channels, sizes[i]);
  if (segmentation != nullptr) { /* the plans of the waves count chains per wave; the batch's count is refused up front */
    std::vector<AADHipStreamDesc> streams(num_streams);
    for (uint32_t i = 0; i < num_streams; i++) streams[i] = AADHipStreamDesc{0, 0, 0, num_samples[i], 0};
    if (aad::segment_chain_count(streams.data(), num_streams, h.num_samples_per_block, segmentation->segment_blocks) > UINT32_MAX) {
      snprintf(ctx->last_error, sizeof(ctx->last_error), "segmented reconstruction: more than %u chains", (unsigned)UINT32_MAX);
      return AAD_APIRESULT_INVALID_ARGUMENT;
    }
  }
  const uint64_t chunk = staging_chunk(ctx);
  uint64_t budget;
  if (!wave_budget(ctx, &budget)) return AAD_APIRESULT_NG;
  AADApiResult rc = AAD_APIRESULT_OK;
  for (uint32_t first = 0; first < num_streams && rc == AAD_APIRESULT_OK;) {
    uint32_t n = 0;
    uint64_t sum = 0;
    while (first + n < num_streams && (n == 0 || sum + footprint[first + n] <= budget)) sum += footprint[first + n++]; /* a stream alone is always tried */
    rc = reconstruct_wave(ctx, parameter, segmentation, n, pcm + first, num_samples + first, output_kind, out_pcm ? out_pcm + first : nullptr,
                          stats ? stats + first : nullptr, chunk);
    first += n;
  }
  return rc;
}

} /* namespace */

AADApiResult AADHip_ReconstructBatch(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                     uint32_t num_streams, const int16_t *const *pcm, const uint32_t *num_samples,
                                     int32_t output_kind, int16_t *const *out_pcm, struct AADHipErrorStats *stats)
{
  if (ctx == nullptr || parameter == nullptr || (num_streams != 0 && (pcm == nullptr || num_samples == nullptr)))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  return reconstruct_batch(ctx, parameter, nullptr, num_streams, pcm, num_samples, output_kind, out_pcm, stats);
}

AADApiResult AADHip_SegmentedReconstructBatch(struct AADHipContext *ctx, const struct AADEncodeParameter *parameter,
                                              const struct AADHipSegmentation *segmentation, uint32_t num_streams,
                                              const int16_t *const *pcm, const uint32_t *num_samples, int32_t output_kind,
                                              int16_t *const *out_pcm, struct AADHipErrorStats *stats)
{
  if (ctx == nullptr || parameter == nullptr || segmentation == nullptr || segmentation->segment_blocks == 0 ||
      (num_streams != 0 && (pcm == nullptr || num_samples == nullptr)))
    return AAD_APIRESULT_INVALID_ARGUMENT;
  return reconstruct_batch(ctx, parameter, segmentation, num_streams, pcm, num_samples, output_kind, out_pcm, stats);
}

#if AAD_PHASE_TIMING
/* measurement builds only: copy out and reset the phase log of the encode kernel */
uint32_t AADHipDebug_ReadPhaseTimes(uint64_t *out, uint32_t capacity)
{
  uint32_t n = 0, zero = 0;
  uint64_t host[512];
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(aad::g_phase_count), sizeof(n));
  (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(aad::g_phase_times), sizeof(host));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(aad::g_phase_count), &zero, sizeof(zero));
  if (n > capacity) n = capacity;
  memcpy(out, host, sizeof(uint64_t) * n);
  return n;
}
#endif

} /* extern "C" */
