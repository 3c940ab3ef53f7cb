/* aad_convolve.h - the arithmetic of the convolve stage behind a window decode (AADHip_Convolver*, include/aad_hip.h
 * "reverberation"), compiled for the host and for the device: the quantiser that turns a float32 impulse response into int16 taps
 * with a scale exponent, the default delay, the split of a tap into two signed bytes, the byte planes of the matrix B that the FIR
 * kernel multiplies with (aad_convolve_tile.hip.h), the source batch's row length and the per-window resolve, which the resolve
 * kernel (aad_convolve.hip) runs once per window.  A CPU test runs the same functions against a numpy restatement of the
 * definition and a brute force (tests/convolve_driver.cpp, tests/convolve_oracle.py).  Plain C++ with no container, as
 * aad_resample.h. */
#ifndef AAD_CONVOLVE_H
#define AAD_CONVOLVE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define AAD_CONVOLVE_FN __host__ __device__ inline
#else
#define AAD_CONVOLVE_FN inline
#endif

namespace aad {

constexpr uint32_t kConvolveMaxTaps = 32768;          /* K */
constexpr int32_t kConvolveMaxTap = 32639;            /* 0x7F7F: both bytes of convolve_split stay in int8 */
constexpr uint32_t kConvolveMaxScale = 15;            /* q */
constexpr uint32_t kConvolveNoResponse = 0xFFFFFFFFu; /* a lane's response: the row is zeros */

/* ---- response ----------------------------------------------------------------------------------------------------------------- */

/* h_q[k] = rint(h[k] * 2^q), ties to even (the product in double is exact), q the largest of 0..15 with max |h_q| <= 32639; an
 * all-zero response gets 15.  delay < 0: the index of the largest |h_q|, the lowest on ties - the direct path.  False for K outside
 * 1..32768, a tap that is not finite, a tap past the bound at q = 0 and a delay >= K; nothing is written then. */
/* the rule's two halves, for every quantiser of the project (aad_spectrogram.h has the other): the scale exponent of a set of
 * values whose largest magnitude is `most` - rint is odd and monotone: the largest |h_q| is rint of the largest |h| - or -1 when
 * q = 0 does not fit, and a value at that exponent */
inline int32_t convolve_scale(double most)
{
  int32_t q = (int32_t)kConvolveMaxScale;
  while (q >= 0 && !(rint(ldexp(most, q)) <= (double)kConvolveMaxTap)) q--;
  return q;
}
inline int16_t convolve_round(double v, int32_t q) { return (int16_t)(int32_t)rint(ldexp(v, q)); }

inline bool convolve_quantise(const float *h, uint32_t K, int32_t delay, int16_t *taps, uint32_t *q_out, uint32_t *delay_out)
{
  if (h == nullptr || K == 0 || K > kConvolveMaxTaps || (delay >= 0 && (uint32_t)delay >= K)) return false;
  double most = 0;
  for (uint32_t k = 0; k < K; k++) {
    if (!isfinite(h[k])) return false;
    const double a = fabs((double)h[k]);
    most = a > most ? a : most;
  }
  const int32_t q = convolve_scale(most);
  if (q < 0) return false;
  int32_t peak = 0;
  uint32_t at = 0;
  for (uint32_t k = 0; k < K; k++) {
    const int32_t v = convolve_round((double)h[k], q);
    taps[k] = (int16_t)v;
    const int32_t a = v < 0 ? -v : v;
    if (a > peak) {
      peak = a;
      at = k;
    }
  }
  *q_out = (uint32_t)q;
  *delay_out = delay >= 0 ? (uint32_t)delay : at;
  return true;
}

/* h = 256 hh + hl with both in int8: hl the signed low byte.  |h| <= 32639 keeps hh within +-127. */
struct ConvolveBytes {
  int8_t hh, hl;
};
AAD_CONVOLVE_FN ConvolveBytes convolve_split(int16_t h)
{
  const int8_t hl = (int8_t)(uint8_t)((uint16_t)h & 255u);
  return ConvolveBytes{(int8_t)(((int32_t)h - (int32_t)hl) / 256), hl};
}

/* a sample's bytes: x = 256 xh + xl + 128, xh = x >> 8 signed, xl = (x & 255) - 128; a frame the row does not have is x = 0, the
 * pair (0, -128), like any other zero */
AAD_CONVOLVE_FN ConvolveBytes convolve_split_sample(int16_t x)
{
  return ConvolveBytes{(int8_t)(x >> 8), (int8_t)(uint8_t)(((uint16_t)x & 255u) ^ 128u)};
}

/* The FIR kernel's matrix.  With G[t] = h[K - 1 - t] for t < K and 0 elsewhere - the response reversed - and X the span of the
 * source row that starts at the first output's first tap, output n of a block of 256 is sum over t of X[n + t] G[t].  Output
 * n = 16 i + j is element (i, j) of A B, summed over the k-steps s:  A[i][u] = X[16 i + 64 s + u],  B_s[u][j] = G[64 s + u - j],
 * u < 64: the rows of A are runs of the span 16 elements apart, and B_s is a Hankel matrix of the response (in the response's own
 * index: B_s[u][j] = h[K - 1 - 64 s - u + j]), zero where the index leaves the response: 15 taps in front, up to 63 behind.
 * kConvolveStepTaps taps a step, convolve_steps(K) steps. */
constexpr uint32_t kConvolveStepTaps = 64;
constexpr uint32_t kConvolveStepBytes = 2048; /* a step of the planes: hh then hl, each 64 lanes x 16 bytes */
AAD_CONVOLVE_FN uint32_t convolve_steps(uint32_t K) { return (K + 15 + kConvolveStepTaps - 1) / kConvolveStepTaps; }

/* the response's tap behind B_s[u][j], 0 outside it */
inline int16_t convolve_matrix_tap(const int16_t *taps, uint32_t K, uint32_t s, uint32_t u, uint32_t j)
{
  const int64_t t = (int64_t)kConvolveStepTaps * s + u - j;
  return t >= 0 && t < (int64_t)K ? taps[K - 1 - t] : (int16_t)0;
}

/* The byte planes of B as the kernel loads them: step s at planes + s * kConvolveStepBytes, the hh plane then the hl plane, in
 * each lane l's 16 bytes at 16 l: B_s[16 (l >> 4) + e][l & 15], e < 16 - the operand fragment of a 16x16x64 int8 matrix
 * instruction, one aligned 16-byte load a lane.  planes: convolve_steps(K) * kConvolveStepBytes bytes. */
inline void convolve_build_planes(const int16_t *taps, uint32_t K, int8_t *planes)
{
  const uint32_t steps = convolve_steps(K);
  for (uint32_t s = 0; s < steps; s++)
    for (uint32_t l = 0; l < 64; l++)
      for (uint32_t e = 0; e < 16; e++) {
        const ConvolveBytes b = convolve_split(convolve_matrix_tap(taps, K, s, 16 * (l >> 4) + e, l & 15));
        planes[(size_t)s * kConvolveStepBytes + 16 * l + e] = b.hh;
        planes[(size_t)s * kConvolveStepBytes + 1024 + 16 * l + e] = b.hl;
      }
}

/* 128 sum h: what the shift of the samples' low bytes by 128 leaves out of the four byte products */
inline int64_t convolve_bias(const int16_t *taps, uint32_t K)
{
  int64_t sum = 0;
  for (uint32_t k = 0; k < K; k++) sum += taps[k];
  return 128 * sum;
}

/* ---- rows --------------------------------------------------------------------------------------------------------------------- */

/* T_src = T + K_max - 1; false for T == 0 */
AAD_CONVOLVE_FN bool convolve_source_frames(uint32_t frames, uint32_t max_taps, uint64_t *source_frames)
{
  if (frames == 0) return false;
  *source_frames = (uint64_t)frames + max_taps - 1;
  return true;
}

/* one window's lane record: a contiguous torch int32 [N, 2] tensor on the device is the table */
struct ConvolveLane {
  uint32_t response; /* index of the window's response, kConvolveNoResponse: the row is zeros */
  uint32_t shift;    /* first_frame - src_first: the source row's element that is the window's first frame */
};

struct ConvolveResolved {
  uint64_t stream, src_first; /* the source window */
  ConvolveLane lane;
};

/* Window {stream, first_frame} with response index `response` (the int64 of the table read as uint64, so that a negative one is
 * past R).  lead[r] = K_r - 1 - d_r frames of the stream lie in front of the window's first frame under the response's taps; the
 * source window starts that much early, or at frame 0 when the window starts inside the lead, and `shift` says by how much.  A
 * window without a response keeps its own start: its source row is decoded and never read. */
AAD_CONVOLVE_FN ConvolveResolved convolve_resolve(uint64_t stream, uint64_t first_frame, uint64_t response, uint32_t num_responses,
                                                  const uint32_t *lead)
{
  ConvolveResolved r;
  r.stream = stream;
  r.src_first = first_frame;
  r.lane.response = kConvolveNoResponse;
  r.lane.shift = 0;
  if (response >= num_responses) return r;
  const uint64_t before = first_frame < lead[response] ? first_frame : lead[response];
  r.src_first = first_frame - before;
  r.lane.response = (uint32_t)response;
  r.lane.shift = (uint32_t)before;
  return r;
}

/* `count` of a reverberated row (AADHip_ConvolverRunStats): the number of n < Le whose direct-path source element, element
 * shift + n of the source row, the stream had - c_src being the source row's own count (AADHip_WindowDecodePlanRunStats over the
 * source windows), never more than the row's length.  shift + n < c  <=>  n < c - shift.  In 64 bits: shift runs up to 2^32 - 1. */
AAD_CONVOLVE_FN uint64_t convolve_output_count(uint64_t c_src, uint32_t source_frames, uint32_t shift, uint64_t Le)
{
  const uint64_t c = c_src < source_frames ? c_src : source_frames;
  if (c <= shift) return 0;
  return c - shift < Le ? c - shift : Le;
}

/* ---- elements ----------------------------------------------------------------------------------------------------------------- */

/* INT16: clamp(floor((acc + (Q ? 2^(Q-1) : 0)) / 2^Q)); |acc| < 2^45 */
AAD_CONVOLVE_FN int16_t convolve_int16(int64_t acc, uint32_t q)
{
  const int64_t v = (acc + (q ? (int64_t)1 << (q - 1) : 0)) >> q; /* an arithmetic shift: floor */
  return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}

/* FLOAT32: fl32(acc) * 2^-(15 + Q) - the 64-bit integer rounded once to nearest even, then an exact scale */
AAD_CONVOLVE_FN float convolve_float(int64_t acc, uint32_t q)
{
  return (float)acc * __builtin_bit_cast(float, (uint32_t)(127u - 15u - q) << 23);
}

/* ---- tile geometry of the FIR kernel (aad_convolve_tile.hip.h) ------------------------------------------------------------------ */

constexpr uint32_t kConvolveThreads = 256;
constexpr uint32_t kConvolveBlock = 256;     /* outputs of one 16 x 16 accumulator tile */
constexpr uint32_t kConvolveWaveBlocks = 4;  /* accumulator tiles a wave keeps: a fragment of B is loaded once for all of them */
constexpr uint32_t kConvolveTile = (kConvolveThreads / 64) * kConvolveWaveBlocks * kConvolveBlock; /* outputs of a workgroup's tile */
constexpr uint32_t kConvolvePieceSteps = 64; /* k-steps between two stagings of the span */
/* elements of a plane of the span in LDS: the tile's outputs and a piece's taps; the last fragment read ends at
 * (kConvolveTile - 256) + 16 * (15 + 3) + 64 * (kConvolvePieceSteps - 1) + 16, below this */
constexpr uint32_t kConvolveSpan = kConvolveTile + kConvolvePieceSteps * kConvolveStepTaps;

} /* namespace aad */

#endif /* AAD_CONVOLVE_H */
