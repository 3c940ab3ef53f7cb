/* aad_spectrogram.h - the arithmetic of the spectrogram stage (AADHip_Spectrogram*, include/aad_hip.h "spectrogram"), compiled for
 * the host and for the device: the quantiser that turns a window into the int16 cos / -sin matrices of a framed real DFT with one
 * scale exponent, the frame count, the bands of the filters, the column constants, the byte planes of the matrix B that the kernel
 * multiplies with (aad_spectrogram.hip), the tile geometry and the one rule for what a run refuses.  A CPU test runs the same
 * functions against a numpy restatement of the definition (tests/spectrogram_driver.cpp, tests/spectrogram_oracle.py).  Plain C++
 * with no container, as aad_convolve.h, whose quantiser rule and byte splits these functions call. */
#ifndef AAD_SPECTROGRAM_H
#define AAD_SPECTROGRAM_H

#include "aad_convolve.h"

namespace aad {

constexpr uint32_t kSpectrumMaxFft = 4096;
constexpr double kSpectrumMinWeight = 0x1p-60; /* a nonzero filter weight's least magnitude: no product with P is subnormal */

AAD_CONVOLVE_FN uint32_t spectrum_bins(uint32_t n_fft) { return n_fft / 2 + 1; }                 /* B */
AAD_CONVOLVE_FN uint32_t spectrum_steps(uint32_t W) { return (W + kConvolveStepTaps - 1) / kConvolveStepTaps; } /* k-steps */
AAD_CONVOLVE_FN uint32_t spectrum_pairs(uint32_t n_fft) { return (spectrum_bins(n_fft) + 15) / 16; } /* (Re, Im) column tile pairs */

/* 1 <= W <= n_fft <= 4096, H >= 1 */
AAD_CONVOLVE_FN bool spectrum_shape_ok(uint32_t n_fft, uint32_t W, uint32_t H)
{
  return W >= 1 && W <= n_fft && n_fft <= kSpectrumMaxFft && H >= 1;
}

/* ---- coefficients --------------------------------------------------------------------------------------------------------------- */

/* cos_sin[t][k][0] = rint(c[t][k] 2^q), [1] likewise of s:  c = (double)w[t] cos(2 pi ((k t) mod n_fft) / n_fft),
 * s = -(double)w[t] sin(the same angle), the reduction in integers, q convolve_scale's over both matrices together.  False for a
 * shape spectrum_shape_ok refuses, a window value that is not finite and a coefficient past the bound at q = 0; nothing is written
 * then.  cos_sin: W * B * 2 elements. */
inline bool spectrum_quantise(const float *window, uint32_t n_fft, uint32_t W, int16_t *cos_sin, uint32_t *q_out)
{
  if (window == nullptr || !spectrum_shape_ok(n_fft, W, 1)) return false;
  for (uint32_t t = 0; t < W; t++)
    if (!isfinite(window[t])) return false;
  const uint32_t B = spectrum_bins(n_fft);
  double *const table = new double[2 * (size_t)n_fft]; /* cos then sin of 2 pi m / n_fft */
  for (uint32_t m = 0; m < n_fft; m++) {
    const double angle = 2.0 * M_PI * (double)m / (double)n_fft;
    table[m] = cos(angle);
    table[n_fft + m] = sin(angle);
  }
  double most = 0;
  for (uint32_t t = 0; t < W; t++)
    for (uint32_t k = 0; k < B; k++) {
      const uint32_t m = (k * t) % n_fft; /* < 2^24: no wrap */
      const double c = fabs((double)window[t] * table[m]), s = fabs((double)window[t] * table[n_fft + m]);
      most = c > most ? c : most;
      most = s > most ? s : most;
    }
  const int32_t q = convolve_scale(most);
  if (q >= 0) {
    for (uint32_t t = 0; t < W; t++)
      for (uint32_t k = 0; k < B; k++) {
        const uint32_t m = (k * t) % n_fft;
        cos_sin[2 * ((size_t)t * B + k)] = convolve_round((double)window[t] * table[m], q);
        cos_sin[2 * ((size_t)t * B + k) + 1] = convolve_round(-(double)window[t] * table[n_fft + m], q);
      }
    *q_out = (uint32_t)q;
  }
  delete[] table;
  return q >= 0;
}

/* ---- frames --------------------------------------------------------------------------------------------------------------------- */

/* F = 1 + (T - W) / H; false for T < W */
AAD_CONVOLVE_FN bool spectrum_frames(uint32_t T, uint32_t W, uint32_t H, uint32_t *F)
{
  if (T < W || W == 0 || H == 0) return false;
  *F = 1 + (T - W) / H;
  return true;
}

/* ---- filters -------------------------------------------------------------------------------------------------------------------- */

/* filter j: its first and last nonzero weight and where weights lo ... hi lie in the packed array; an all-zero filter is
 * lo = B, hi = 0 and no weight */
struct SpectrumBand {
  uint32_t lo, hi, offset;
};

/* bands[M] and the number of packed weights; false for a weight that is not finite or a nonzero one below 2^-60 in magnitude */
inline bool spectrum_bands(const float *filters, uint32_t M, uint32_t B, SpectrumBand *bands, uint64_t *total)
{
  uint64_t at = 0;
  for (uint32_t j = 0; j < M; j++) {
    SpectrumBand b = {B, 0, (uint32_t)at};
    for (uint32_t k = 0; k < B; k++) {
      const float w = filters[(size_t)j * B + k];
      if (!isfinite(w) || (w != 0 && fabs((double)w) < kSpectrumMinWeight)) return false;
      if (w != 0) {
        b.lo = b.lo == B ? k : b.lo;
        b.hi = k;
      }
    }
    bands[j] = b;
    if (b.lo != B) at += b.hi - b.lo + 1;
    if (at > UINT32_MAX) return false;
  }
  *total = at;
  return true;
}

/* the weights band after band: zeros inside a band are weights like any other */
inline void spectrum_pack_weights(const float *filters, uint32_t M, uint32_t B, const SpectrumBand *bands, float *packed)
{
  for (uint32_t j = 0; j < M; j++)
    for (uint32_t k = bands[j].lo; k <= bands[j].hi && bands[j].lo != B; k++) packed[bands[j].offset + k - bands[j].lo] = filters[(size_t)j * B + k];
}

/* The filters a column tile pair touches, in the filters' order: first[c] ... first[c + 1] of `list` are the filters with a bin in
 * 16 c ... 16 c + 15; an all-zero filter is listed under pair 0, where the kernel writes its +0.  list null: first alone, for the
 * list's size first[pairs]. */
inline void spectrum_tile_lists(const SpectrumBand *bands, uint32_t M, uint32_t B, uint32_t pairs, uint32_t *first, uint32_t *list)
{
  uint32_t at = 0;
  for (uint32_t c = 0; c < pairs; c++) {
    first[c] = at;
    for (uint32_t j = 0; j < M; j++) {
      const bool empty = bands[j].lo == B;
      if (empty ? c == 0 : (bands[j].lo <= 16 * c + 15 && bands[j].hi >= 16 * c)) {
        if (list != nullptr) list[at] = j;
        at++;
      }
    }
  }
  first[pairs] = at;
}

/* ---- the matrix ----------------------------------------------------------------------------------------------------------------- */

/* Frame f of a row is row f of A, the run of the row that starts at f H, and B is the two coefficient matrices side by side in
 * column tiles of 16: tile 2 c holds the cos columns of bins 16 c ... 16 c + 15 and tile 2 c + 1 their -sin columns, so Re and Im
 * of a bin are the same column of two tiles and a lane holds both.  k-step s covers t = 64 s ... 64 s + 63.  Rows t >= W of the
 * last step and columns past B are zero. */
constexpr uint32_t kSpectrumStepBytes = kConvolveStepBytes; /* a step of a column tile: hh then hl, each 64 lanes x 16 bytes */

/* element [t][column j of tile ct] of B */
inline int16_t spectrum_matrix_element(const int16_t *cos_sin, uint32_t W, uint32_t B, uint32_t ct, uint32_t t, uint32_t j)
{
  const uint32_t k = 16 * (ct >> 1) + j;
  return t < W && k < B ? cos_sin[2 * ((size_t)t * B + k) + (ct & 1u)] : (int16_t)0;
}

AAD_CONVOLVE_FN uint64_t spectrum_plane_bytes(uint32_t n_fft, uint32_t W)
{
  return (uint64_t)2 * spectrum_pairs(n_fft) * spectrum_steps(W) * kSpectrumStepBytes;
}

/* The byte planes as the kernel loads them: column tile ct's step s at planes + (ct * steps + s) * kSpectrumStepBytes, the hh
 * plane then the hl plane, lane l's 16 bytes at 16 l: element [64 s + 16 (l >> 4) + e][l & 15], e < 16 - convolve_build_planes'
 * operand order, one aligned 16-byte load a lane.  planes: spectrum_plane_bytes. */
inline void spectrum_build_planes(const int16_t *cos_sin, uint32_t n_fft, uint32_t W, int8_t *planes)
{
  const uint32_t B = spectrum_bins(n_fft), tiles = 2 * spectrum_pairs(n_fft), steps = spectrum_steps(W);
  for (uint32_t ct = 0; ct < tiles; ct++)
    for (uint32_t s = 0; s < steps; s++)
      for (uint32_t l = 0; l < 64; l++)
        for (uint32_t e = 0; e < 16; e++) {
          const ConvolveBytes b = convolve_split(spectrum_matrix_element(cos_sin, W, B, ct, 64 * s + 16 * (l >> 4) + e, l & 15));
          const size_t at = ((size_t)ct * steps + s) * kSpectrumStepBytes + 16 * l + e;
          planes[at] = b.hh;
          planes[at + 1024] = b.hl;
        }
}

/* 128 sum over t of the column: what the shift of the samples' low bytes by 128 leaves out of the four byte products.
 * consts[part * 16 * pairs + k], part 0 the cos and 1 the -sin matrix, zero for k >= B */
inline void spectrum_column_constants(const int16_t *cos_sin, uint32_t n_fft, uint32_t W, int64_t *consts)
{
  const uint32_t B = spectrum_bins(n_fft), pitch = 16 * spectrum_pairs(n_fft);
  for (uint32_t i = 0; i < 2 * pitch; i++) consts[i] = 0;
  for (uint32_t t = 0; t < W; t++)
    for (uint32_t k = 0; k < B; k++)
      for (uint32_t part = 0; part < 2; part++) consts[part * pitch + k] += 128 * (int64_t)cos_sin[2 * ((size_t)t * B + k) + part];
}

/* ---- elements ------------------------------------------------------------------------------------------------------------------- */

/* The element of an exact sum that lies in the kernel's three accumulators, S = 65536 a0 + 256 a1 + a2 + c: fl32(S) 2^-(15 + q),
 * convolve_float's value, by way of double - every term and every partial sum is an integer below 2^53 times the power of two
 * `scale` = 2^-(15 + q), so the double arithmetic is exact whether or not it fuses, and the conversion to float32 is the one
 * rounding, to nearest even; no result but 0 lies below 2^-30, so none is subnormal.  c_scaled: (double)c * scale. */
AAD_CONVOLVE_FN double spectrum_scale(uint32_t q) { return __builtin_bit_cast(double, (uint64_t)(1023u - 15u - q) << 52); }
AAD_CONVOLVE_FN float spectrum_element(int32_t a0, int32_t a1, int32_t a2, double c_scaled, double scale)
{
  return (float)((double)a0 * (65536.0 * scale) + ((double)a1 * (256.0 * scale) + ((double)a2 * scale + c_scaled)));
}

/* P = fl32(fl32(re re) + fl32(im im)): two multiplies and one add, never an fma */
AAD_CONVOLVE_FN float spectrum_power(float re, float im)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
#else
  volatile float a = re * re, b = im * im; /* the host's compiler may not fuse across a volatile */
  return a + b;
#endif
}

/* ---- tile geometry of the kernel (aad_spectrogram.hip) -------------------------------------------------------------------------- */

constexpr uint32_t kSpectrumThreads = 256;
constexpr uint32_t kSpectrumWaveBlocks = 4; /* 16-frame blocks a wave keeps: a fragment of B is loaded once for all of them */
constexpr uint32_t kSpectrumTileFrames = (kSpectrumThreads / 64) * kSpectrumWaveBlocks * 16; /* the most frames of a workgroup's tile */
constexpr uint32_t kSpectrumSpan = 65536;      /* the most elements of a plane of the tile's samples in LDS */
constexpr uint32_t kSpectrumExchangePitch = 17; /* floats between two frames' 16 powers in the hand-off buffer: no bank shared */
static_assert(kSpectrumTileFrames == kSpectrumThreads, "the mel hand-off: a thread per frame of the tile");

/* How a tile's samples lie in LDS.  Frame i of the tile starts at element i * pitch of a plane, so a fragment read is the 16
 * bytes at i * pitch + 64 s + 16 g - aligned, pitch being a multiple of 16.  A hop that is a multiple of 16 stages the tile's
 * span of the row once, pitch = H; any other hop, or one whose span of 16 frames passes kSpectrumSpan, stages frame by frame,
 * pitch = 64 * steps: an element of the row is then written once per frame that covers it.  tile_frames: the frames of a
 * workgroup's tile, the largest multiple of 16 up to kSpectrumTileFrames whose plane fits; plane_elements: of such a tile. */
struct SpectrumGeometry {
  uint32_t pitch, tile_frames, frame_major, plane_elements;
};
AAD_CONVOLVE_FN uint32_t spectrum_fit(uint64_t pitch, uint32_t step_elements)
{
  const uint64_t n = (kSpectrumSpan - step_elements) / pitch + 1;
  return (uint32_t)(n < kSpectrumTileFrames ? n : kSpectrumTileFrames) & ~15u;
}
AAD_CONVOLVE_FN SpectrumGeometry spectrum_geometry(uint32_t W, uint32_t H)
{
  const uint32_t step_elements = kConvolveStepTaps * spectrum_steps(W); /* <= 4096 */
  SpectrumGeometry g;
  g.frame_major = H % 16 != 0 || spectrum_fit(H, step_elements) < 16;
  g.pitch = g.frame_major ? step_elements : H;
  g.tile_frames = spectrum_fit(g.pitch, step_elements); /* frame by frame: 1024 / steps >= 16 */
  g.plane_elements = (g.tile_frames - 1) * g.pitch + step_elements;
  return g;
}
/* bytes of LDS a launch asks for: the two planes and, with filters, the hand-off buffer */
AAD_CONVOLVE_FN uint32_t spectrum_lds_bytes(const SpectrumGeometry &g, bool filters)
{
  return 2 * g.plane_elements + (filters ? 4 * kSpectrumExchangePitch * kSpectrumTileFrames : 0);
}

/* ---- a run ---------------------------------------------------------------------------------------------------------------------- */

struct SpectrumRows {
  bool ok;
  uint32_t num_frames; /* F */
  uint32_t tiles;      /* workgroups of a row */
  uint64_t items;      /* num_rows * tiles */
};

/* A run over int16 rows of `frames` elements, row_pitch apart, into float32 [num_rows, F, columns] - pointers come in as
 * addresses.  Refused: a null pointer, rows off 2-byte or out off 4-byte alignment, frames < W, row_pitch < frames, and the rows'
 * bytes, the output's bytes or num_rows * tiles past 64 bits. */
inline SpectrumRows spectrum_rows(uint64_t num_rows, uint64_t rows, uint64_t row_pitch, uint32_t frames, uint64_t out, uint32_t W,
                                  uint32_t H, uint32_t columns, uint32_t tile_frames)
{
  SpectrumRows r = {false, 0, 0, 0};
  uint64_t n = 0;
  if (rows == 0 || out == 0 || (rows & 1u) != 0 || (out & 3u) != 0 || row_pitch < frames || !spectrum_frames(frames, W, H, &r.num_frames))
    return r;
  r.tiles = (r.num_frames - 1) / tile_frames + 1;
  r.ok = !__builtin_mul_overflow(num_rows, row_pitch, &n) && !__builtin_mul_overflow(n, (uint64_t)2, &n) &&
         !__builtin_mul_overflow(num_rows, (uint64_t)r.num_frames, &n) && !__builtin_mul_overflow(n, (uint64_t)columns, &n) &&
         !__builtin_mul_overflow(n, (uint64_t)4, &n) && !__builtin_mul_overflow(num_rows, (uint64_t)r.tiles, &r.items);
  return r;
}

/* ---- a mix (include/aad_hip.h "spectrogram", paragraph "mix") -------------------------------------------------------------------- */

/* The staged sample of AADHip_SpectrogramRunMix: m = fl32(ga a), inside b's span m = fl32(m + fl32(gb b)) - two multiplies and one
 * add, never a fused one - then 0 for a NaN, else the nearest integer, ties to even, clamped to int16: an infinite m gives the
 * rail.  The conversions of a and b are exact.  The kernel's stager (aad_spectrogram_mix.hip) and tests/spectrogram_mix_driver.cpp
 * compile this one function. */
AAD_CONVOLVE_FN int16_t spectrum_mix_sample(float ga, int16_t a, float gb, int16_t b, bool inside)
{
#if defined(__HIP_DEVICE_COMPILE__)
  float m = __fmul_rn(ga, (float)a);
  if (inside) m = __fadd_rn(m, __fmul_rn(gb, (float)b));
#else
  volatile float pa = ga * (float)a, pb = gb * (float)b; /* the host's compiler may not fuse across a volatile */
  float m = pa;
  if (inside) m = pa + pb;
#endif
  if (!(m == m)) return 0;
  const float r = rintf(m); /* to nearest even: no unit changes the rounding mode */
  return (int16_t)(r < -32768.0f ? -32768 : r > 32767.0f ? 32767 : (int32_t)r);
}

/* Le of "Window decode with a span": 0 for o >= T, else min(L, T - o) - the comparison first, no sum of two 64-bit values */
AAD_CONVOLVE_FN uint32_t spectrum_mix_span(uint64_t L, uint64_t o, uint32_t T)
{
  if (o >= T) return 0;
  return L < T - o ? (uint32_t)L : (uint32_t)(T - o);
}

/* A mix run: spectrum_rows for both row batches, and rows_per_gain C >= 1 that divides num_rows; gain tables (0: none) on 4-byte
 * and the span table (0: none) on 8-byte alignment, num_rows / C records each, whose bytes lie within 64 bits. */
inline SpectrumRows spectrum_mix_rows(uint64_t num_rows, uint64_t rows_a, uint64_t row_pitch_a, uint64_t rows_b, uint64_t row_pitch_b,
                                      uint32_t rows_per_gain, uint64_t gain_a, uint64_t gain_b, uint64_t spans, uint32_t frames, uint64_t out,
                                      uint32_t W, uint32_t H, uint32_t columns, uint32_t tile_frames)
{
  SpectrumRows r = spectrum_rows(num_rows, rows_a, row_pitch_a, frames, out, W, H, columns, tile_frames);
  uint64_t n = 0;
  r.ok = r.ok && spectrum_rows(num_rows, rows_b, row_pitch_b, frames, out, W, H, columns, tile_frames).ok && rows_per_gain != 0 &&
         num_rows % rows_per_gain == 0 && (gain_a & 3u) == 0 && (gain_b & 3u) == 0 && (spans & 7u) == 0 &&
         !__builtin_mul_overflow(num_rows / rows_per_gain, (uint64_t)16, &n);
  return r;
}

} /* namespace aad */

#endif /* AAD_SPECTROGRAM_H */
