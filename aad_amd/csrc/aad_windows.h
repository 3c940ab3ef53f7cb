/* aad_windows.h - the arithmetic of a window reconstruct run (AADHip_WindowReconstructPlanRun, include/aad_hip.h), compiled for the
 * host and for the device: the resolve kernel (aad_window_reconstruct.hip) turns a window table in device memory into the lanes of
 * an encoder launch with these functions, and a CPU test runs the same functions against the host builders of aad_segments.h
 * (tests/test_window_reconstruct_host.py).  The segment rule itself (segment_count, segment_cut) is stated here once:
 * build_segment_chains takes it from here too.  Plain C++ with no container, as aad_pcm_convert.h. */
#ifndef AAD_WINDOWS_H
#define AAD_WINDOWS_H

#include <stdint.h>

#include "../../include/aad_hip.h"

#if defined(__HIPCC__)
#define AAD_WINDOWS_FN __host__ __device__ inline
#else
#define AAD_WINDOWS_FN inline
#endif

namespace aad {

/* ---- the segment rule (include/aad_hip.h "segmented encode") ---------------------------------------------------------------- */

/* chains of a stream of n frames: ceil(B / L), B = ceil(n / spb); one for a stream of less than a block */
AAD_WINDOWS_FN uint64_t segment_count(uint64_t n, uint32_t spb, uint32_t segment_blocks)
{
  const uint64_t b = (n + spb - 1) / spb;
  return b == 0 ? 1u : (b + segment_blocks - 1) / segment_blocks;
}

/* segment s of a stream of n frames: the chain encodes frames [first_frame, end_frame) as a fresh encoder, its first
 * warmup_blocks blocks are discarded and block first_block of the stream is the first it encodes (a warm-up block, if any) */
struct SegmentCut {
  uint64_t first_frame, end_frame;
  uint64_t first_block;
  uint32_t warmup_blocks;
};
AAD_WINDOWS_FN SegmentCut segment_cut(uint64_t n, uint32_t spb, uint32_t segment_blocks, uint32_t warmup_blocks, uint64_t s)
{
  const uint64_t L = segment_blocks, kept = s * L, w = warmup_blocks < kept ? warmup_blocks : kept;
  SegmentCut c;
  c.first_frame = (kept - w) * spb;
  c.end_frame = (s + 1) * L * spb < n ? (s + 1) * L * spb : n;
  c.first_block = kept - w;
  c.warmup_blocks = (uint32_t)w;
  return c;
}

/* ---- windows ---------------------------------------------------------------------------------------------------------------- */

/* len_w: the frames of window {stream, first_frame} that exist, at most `frames`.  0 for a stream index past the table and a start
 * at or past the stream's end - which covers huge and wrapped-negative values - and then no descriptor field is looked at. */
AAD_WINDOWS_FN uint32_t window_length(uint64_t stream, uint64_t first_frame, uint32_t frames, uint64_t num_sources,
                                      const AADHipStreamDesc *sources)
{
  if (stream >= num_sources) return 0;
  const uint64_t n = sources[stream].num_samples;
  if (first_frame >= n) return 0;
  return n - first_frame < frames ? (uint32_t)(n - first_frame) : frames;
}

/* what every window of a run shares */
struct WindowGeometry {
  uint32_t frames;            /* T */
  uint32_t spb;               /* samples per block */
  uint32_t segment_blocks;    /* L, 0: unsegmented (one lane per window) */
  uint32_t warmup_blocks;     /* W */
  uint32_t chains_per_window; /* lanes per window: window_chains(frames, spb, L) */
  uint32_t reserved;
  uint64_t image_stride;      /* bytes from window w's image to window w + 1's */
  uint64_t out_stream_stride; /* elements from window w's channel-0 row to window w + 1's */
};

/* lanes per window of the uniform launch: the chains of a full window of T frames (1 when unsegmented) */
AAD_WINDOWS_FN uint64_t window_chains(uint32_t frames, uint32_t spb, uint32_t segment_blocks)
{
  return segment_blocks == 0 ? 1u : segment_count(frames, spb, segment_blocks);
}

/* One lane of the launch: chain k of window w.  The fields are ChainDesc's (aad_segments.h) plus the lane's entries of the output
 * base and statistics tables; an unsegmented run's lane is the StreamDesc {pcm_offset, data_offset, 0, num_frames}. */
struct WindowLane {
  uint64_t pcm_offset;  /* element of channel 0's source row that starts the lane's first encoded frame */
  uint64_t data_offset; /* w * image_stride */
  uint64_t first_block;
  uint64_t out_base;    /* element of the output that holds channel 0's sample of the lane's first frame */
  uint32_t num_frames;
  uint32_t warmup_blocks;
  uint32_t header_samples; /* len_w */
  uint32_t writes_header;
  uint32_t stats_stream;   /* w: the lane's records are window w's */
};

/* source_offset: the source stream's pcm_offset (anything when len == 0: nothing is read); len: window_length().  For
 * k < segment_count(len) this is chain k of a single stream of len frames at source_offset + first_frame, as build_segment_chains,
 * reconstruct_output_bases and chain_streams give it for stream w of a batch; the chains behind those, which the uniform launch
 * brings along, encode nothing and write no header. */
AAD_WINDOWS_FN WindowLane window_lane(const WindowGeometry &g, uint64_t w, uint32_t k, uint64_t source_offset, uint64_t first_frame,
                                      uint32_t len)
{
  WindowLane r;
  r.pcm_offset = len != 0 ? source_offset + first_frame : 0;
  r.data_offset = w * g.image_stride;
  r.first_block = 0;
  r.out_base = w * g.out_stream_stride;
  r.num_frames = 0;
  r.warmup_blocks = 0;
  r.header_samples = len;
  r.writes_header = 0;
  r.stats_stream = (uint32_t)w;
  if (g.segment_blocks == 0) {
    r.num_frames = len;
    r.writes_header = 1;
    return r;
  }
  if (k >= segment_count(len, g.spb, g.segment_blocks)) return r; /* padding: total == 0, no warm-up, no header */
  const SegmentCut c = segment_cut(len, g.spb, g.segment_blocks, g.warmup_blocks, k);
  r.pcm_offset += c.first_frame;
  r.first_block = c.first_block;
  r.out_base += c.first_block * g.spb;
  r.num_frames = (uint32_t)(c.end_frame - c.first_frame);
  r.warmup_blocks = c.warmup_blocks;
  r.writes_header = k == 0 ? 1u : 0u;
  return r;
}

/* ---- what a run refuses (host) ------------------------------------------------------------------------------------------------ */

/* lanes of a run, N * chains per window; false past UINT32_MAX (the kernels index lanes with 32 bits) */
inline bool window_lane_count(uint64_t num_windows, uint32_t frames, uint32_t spb, uint32_t segment_blocks, uint64_t *lanes)
{
  uint64_t n = 0;
  if (spb == 0 || __builtin_mul_overflow(num_windows, window_chains(frames, spb, segment_blocks), &n) || n > UINT32_MAX) return false;
  *lanes = n;
  return true;
}

/* the images of a run: window w's at w * image_stride, each with room for a full window's image_bytes
 * (AADHip_CalculateEncodedSize of T frames), all inside 64 bits */
inline bool window_images_ok(uint64_t num_windows, uint64_t image_stride, uint64_t image_bytes)
{
  if (num_windows > 1 && image_stride < image_bytes) return false;
  uint64_t end = 0;
  return num_windows == 0 || !(__builtin_mul_overflow(num_windows - 1, image_stride, &end) || __builtin_add_overflow(end, image_bytes, &end));
}

/* the source table of a plan: C > 1 needs channel_stride >= the longest stream, and every row ends inside 64 bits of elements and
 * bytes (pcm_offset + (C - 1) channel_stride + num_samples, as AADHip_PlanarEncodePlanCreate asks) */
inline bool window_sources_ok(uint32_t channels, uint64_t channel_stride, uint32_t elem_bytes, uint32_t num_sources,
                              const AADHipStreamDesc *sources)
{
  if (channels == 0) return false;
  for (uint32_t i = 0; i < num_sources; i++) {
    if (channels > 1 && channel_stride < sources[i].num_samples) return false;
    uint64_t span = 0, end = 0, bytes = 0;
    if (__builtin_mul_overflow((uint64_t)(channels - 1), channel_stride, &span) ||
        __builtin_add_overflow(span, (uint64_t)sources[i].num_samples, &span) || __builtin_add_overflow(sources[i].pcm_offset, span, &end) ||
        __builtin_mul_overflow(end, (uint64_t)elem_bytes, &bytes))
      return false;
  }
  return true;
}

} /* namespace aad */

#endif /* AAD_WINDOWS_H */
