/* aad_fir_stage.h - what the FIR stages behind a window decode (resample, convolve: aad_fir_stage.hip) refuse of a call's
 * arguments, as plain functions over integers - pointers come in as addresses - that a host test holds to the arithmetic. */
#ifndef AAD_FIR_STAGE_H
#define AAD_FIR_STAGE_H

#include "../../include/aad_hip.h" /* and stdint.h */

namespace aad {

struct FirRows {
  bool ok;
  uint64_t rows;  /* num_windows * channels */
  uint32_t tiles; /* ceil(frames / tile): the workgroups of a row */
};

/* A FIR run over int16 rows [num_windows, channels, source_frames] into rows [num_windows, channels, frames] of `elem` (2 or 4)
 * bytes an element, a workgroup per `tile` output frames; needed_source_frames: the stage's, of aad_resample.h or aad_convolve.h;
 * out_optional: a statistics run.  Refused past the first condition: a row count, a batch's bytes or rows * tiles past 64 bits. */
inline FirRows fir_rows(uint64_t num_windows, uint32_t channels, uint32_t frames, uint32_t source_frames, uint32_t needed_source_frames,
                        uint64_t elem, uint64_t src, uint64_t lanes, uint64_t out, bool out_optional, uint32_t tile)
{
  FirRows f = {false, 0, 0};
  uint64_t n = 0;
  if (channels == 0 || frames == 0 || source_frames < needed_source_frames || src == 0 || lanes == 0 || (out == 0 && !out_optional) ||
      (src & 1u) != 0 || (lanes & 3u) != 0 || (out & (elem - 1)) != 0)
    return f;
  f.tiles = (frames - 1) / tile + 1;
  f.ok = !__builtin_mul_overflow(num_windows, (uint64_t)channels, &f.rows) && !__builtin_mul_overflow(f.rows, (uint64_t)frames, &n) &&
         !__builtin_mul_overflow(n, elem, &n) && !__builtin_mul_overflow(f.rows, (uint64_t)source_frames, &n) &&
         !__builtin_mul_overflow(n, (uint64_t)2, &n) && !__builtin_mul_overflow(f.rows, (uint64_t)f.tiles, &n);
  return f;
}

/* The tables of a Resolve: windows, source_windows and the selector (per window the variant or response; it alone may be null)
 * on 8-byte, the lanes on 4-byte boundaries.  The resolve kernel's grid holds INT32_MAX blocks of 256 windows. */
inline bool fir_resolve_ok(uint64_t num_windows, uint64_t windows, uint64_t selector, uint64_t source_windows, uint64_t lanes)
{
  return windows != 0 && source_windows != 0 && lanes != 0 && num_windows <= (uint64_t)INT32_MAX * 256u &&
         ((windows | selector | source_windows) & 7u) == 0 && (lanes & 3u) == 0;
}

/* What a run with gain refuses on top of fir_rows; either table may be null */
inline bool fir_gain_ok(int32_t sample_type, int32_t mode, uint64_t gain, uint64_t spans)
{
  return sample_type != AAD_HIP_SAMPLE_INT16 && (mode == AAD_HIP_WINDOW_GAIN_STORE || mode == AAD_HIP_WINDOW_GAIN_ADD) &&
         (gain & 3u) == 0 && (spans & 7u) == 0;
}

} /* namespace aad */

#endif /* AAD_FIR_STAGE_H */
