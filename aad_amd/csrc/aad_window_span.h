/* aad_window_span.h - the arithmetic of a window decode run with spans (AADHip_WindowDecodePlanRunPlaced, ...RunPlacedStats,
 * include/aad_hip.h), compiled for the host and for the device: window_lane's PLACED mode (aad_decode_window.hip.h) takes the
 * clip of a span, its crop range and its fill tile from these functions, and a CPU test runs the same functions against a brute
 * force over every element of a row (tests/window_span_driver.cpp, tests/test_window_placed_host.py).  Plain C++ with no
 * container, as aad_windows.h. */
#ifndef AAD_WINDOW_SPAN_H
#define AAD_WINDOW_SPAN_H

#include <stdint.h>

#if defined(__HIPCC__)
#define AAD_WINDOW_SPAN_FN __host__ __device__ inline
#else
#define AAD_WINDOW_SPAN_FN inline
#endif

namespace aad {

/* Le: the frames of span (L, o) that a row of T elements takes.  The comparison comes first, so no sum of two 64-bit values is
 * formed and huge or wrapped values clip like any other */
AAD_WINDOW_SPAN_FN uint64_t window_span_frames(uint64_t num_frames, uint64_t out_frame, uint32_t frames)
{
  if (out_frame >= frames) return 0;
  const uint64_t room = frames - out_frame;
  return num_frames < room ? num_frames : room;
}

/* Lane k of a window decodes block first_frame / spb + k of its stream; phase = first_frame % spb, so sample i of that block is
 * crop index base + i.  The lane keeps the crop indices [lo, hi) - hi <= lo: none - of a crop of `frames` frames; `past`: the
 * block lies behind the crop's last one and the lane decodes nothing */
struct WindowCropRange {
  int64_t base, lo, hi;
  bool past;
};
AAD_WINDOW_SPAN_FN WindowCropRange window_crop_range(uint32_t k, uint64_t spb, uint64_t phase, uint64_t frames)
{
  const uint64_t kspb = (uint64_t)k * spb;
  WindowCropRange r;
  r.past = kspb >= frames + phase;
  r.base = (int64_t)kspb - (int64_t)phase;
  r.lo = r.base > 0 ? r.base : 0;
  r.hi = r.base + (int64_t)spb < (int64_t)frames ? r.base + (int64_t)spb : (int64_t)frames;
  return r;
}

/* The fill of lane k under STORE: the tile the lane would own in a run without spans, [k * spb - phase, (k + 1) * spb - phase)
 * cut to the row [0, T), minus the span [o, o + Le) - the piece in front of the span and the piece behind it, row elements
 * [lo[j], hi[j]), hi <= lo: empty.  Together at most spb elements.  The K lanes' tiles cover [0, T): K is planned from a
 * samples-per-block value <= spb (window_blocks_spanned), so K * spb - phase >= T - 1 + spb - phase >= T. */
struct WindowFillTile {
  int64_t lo[2], hi[2];
};
AAD_WINDOW_SPAN_FN WindowFillTile window_fill_tile(uint32_t k, uint64_t spb, uint64_t phase, uint32_t frames, uint64_t out_frame,
                                                   uint64_t span_frames)
{
  const int64_t start = (int64_t)((uint64_t)k * spb) - (int64_t)phase, end = start + (int64_t)spb;
  const int64_t lo = start > 0 ? start : 0, hi = end < (int64_t)frames ? end : (int64_t)frames;
  /* an empty span takes nothing out, wherever it lies (out_frame may be any 64-bit value then) */
  const int64_t s0 = span_frames ? (int64_t)out_frame : hi, s1 = span_frames ? (int64_t)(out_frame + span_frames) : hi;
  WindowFillTile t;
  t.lo[0] = lo;
  t.hi[0] = hi < s0 ? hi : s0;
  t.lo[1] = lo > s1 ? lo : s1;
  t.hi[1] = hi;
  return t;
}

} /* namespace aad */

#endif /* AAD_WINDOW_SPAN_H */
