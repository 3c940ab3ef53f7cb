/* aad_hip_context.hip.h - library-private: the context behind struct AADHipContext and the few host helpers that every unit
 * with entry points of include/aad_hip.h needs (aad_hip_engine.hip, aad_fir_stage.hip).  Host code alone. */
#ifndef AAD_HIP_CONTEXT_HIP_H
#define AAD_HIP_CONTEXT_HIP_H

#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/aad_hip.h"
#include "aad_launch.h" /* and aad_launch_policy.h */

/* grow-only pinned-host + device buffer pair used by the host-memory calls.  Everything a run
 * needs (stream table, block prefix, carried state, payload) is laid out in ONE pinned block and
 * crosses PCIe in ONE copy each way: a copy per stream from pageable memory cost ~10 us apiece
 * (20 ms for a 1000-stream batch), and per-call hipMalloc / table upload / extra synchronisations
 * cost more than the kernels themselves (round 1: 2.9 ms per call for a 0.075 ms kernel). */
struct Staging {
  void *host = nullptr, *dev = nullptr;
  size_t cap = 0;
};

struct StagingPool; /* aad_hip_engine.hip: the helper threads of the host-memory calls */

struct AADHipContext {
  int device;
  hipStream_t stream;
  bool owns_stream;
  char last_error[256];
  /* double-buffered so that a big batch can be cut into chunks: while chunk k is on the device the
   * host fills chunk k+1's input block and drains chunk k-1's output block */
  Staging in[2], out[2];
  hipEvent_t chunk_done[2];
  hipEvent_t piece_done[3]; /* the earlier pieces of a one-tile decode's output copy */
  /* a cut batch runs its copies on streams of their own, so that tile k+1 goes up and tile k-1
   * comes down while tile k computes */
  hipStream_t up_stream, down_stream;
  hipEvent_t uploaded[2], computed[2];
  bool have_events, have_pipeline;
  /* device blocks of the host-memory reconstruction (grow-only): the wave's PCM, its output + statistics */
  void *d_rc_in, *d_rc_out;
  size_t rc_in_capacity, rc_out_capacity;
  /* device-only scratch of the reconstruction modes (the .aad images never leave HBM) */
  void *d_scratch;
  size_t scratch_capacity;
  /* scratch of the split decoder (dequantised differences), grow-only and shared by every decode
   * plan of the context: their runs are ordered by the context's one stream */
  int32_t *d_residual;
  uint64_t residual_capacity;
  /* scratch of the dual trial search (three block-sized slots per stream, aad_encode.hip.h
   * encode_block_dual), grow-only, shared by the context's encode launches like d_residual */
  uint8_t *d_trial;
  uint64_t trial_capacity;
  /* the images of a window reconstruct run that did not ask for them (the encoders always write images), grow-only likewise */
  uint8_t *d_window_images;
  uint64_t window_images_capacity;
  /* AADHip_ContextSetOption; the defaults come from the environment ONCE, at creation */
  aad::LaunchSignal signal_next; /* AADHip_ContextSignalNextRun: the events the next plan run records around its work (one-shot) */
  bool signal_refused;           /* ROC_SYSTEM_SCOPE_SIGNAL=0 at creation: an event on a dispatch packet is never seen by another queue */
  aad::Device device_info; /* filled once at creation: the launch policy's residency terms */
  aad::Knobs knobs;        /* lane mapping, trial lanes (enum AADHipLaneMapping / AADHipTrialLanes) and the measurement aids */
  int32_t compare_sequential; /* AAD_HIP_OPTION_COMPARE_ORDER: the -c sums always in the reference's order */
  int64_t tile_bytes;      /* 0 = the built-in tile budget of the host-memory path, else that many bytes */
  void *d_state;           /* predictor states of a group of streams between its tiles (host-memory encode) */
  size_t state_capacity;   /* in records */
  int32_t staging_threads; /* 0 = by core count, else the number of threads that copy (1 = the caller alone) */
  StagingPool *pool;    /* staging helper threads, created on demand */
};

inline bool hip_ok(AADHipContext *ctx, hipError_t e, const char *what)
{
  if (e == hipSuccess) return true;
  if (ctx) snprintf(ctx->last_error, sizeof(ctx->last_error), "%s: %s", what, hipGetErrorString(e));
  return false;
}

struct DeviceGuard { /* select the context's device for the calling thread, restore on exit */
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(AADHipContext *ctx)
  {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hip_ok(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  }
  ~DeviceGuard()
  {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <typename T>
bool upload(AADHipContext *ctx, T **dst, const T *src, size_t count)
{
  if (!hip_ok(ctx, hipMalloc((void **)dst, sizeof(T) * (count ? count : 1)), "hipMalloc")) return false;
  if (count == 0) return true;
  /* pageable source: the copy is complete (staged) when this returns */
  return hip_ok(ctx, hipMemcpyAsync(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync") &&
         hip_ok(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

/* the sample types of window decode rows: 2 and 3 are no type, and float16 / bfloat16 exist for window decode alone */
inline bool window_sample_type_ok(int32_t sample_type)
{
  return sample_type == AAD_HIP_SAMPLE_INT16 || sample_type == AAD_HIP_SAMPLE_FLOAT32 || sample_type == AAD_HIP_SAMPLE_FLOAT16 ||
         sample_type == AAD_HIP_SAMPLE_BFLOAT16;
}

#endif /* AAD_HIP_CONTEXT_HIP_H */
