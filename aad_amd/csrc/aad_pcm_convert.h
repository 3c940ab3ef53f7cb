/* aad_pcm_convert.h - the float32 sample of planar encode input (AADHip_PlanarEncodePlanCreate, include/aad_hip.h) as the int16 the
 * encoder sees:
 *   q(v) = 0 for a NaN, else clamp(roundTiesToEven(v * 32768), -32768, 32767)
 * (torch: nan_to_num(x, nan=0).mul(32768).round().clamp(-32768, 32767).to(int16)).  v * 32768 is exact in float32 or overflows to
 * +-inf, which the clamp takes.  The encoder's chunk loads call this as the samples arrive (aad_encode.hip.h PlanarChunk /
 * PlanarRaw); device and host share the header so that a CPU test proves it over every float32 bit pattern
 * (tests/test_planar_host.py, through tests/planar_host_driver.cpp).
 *
 * Written so that no hardware conversion rule decides a value: the NaN is taken out first and the clamp runs on floats, so the
 * float -> int conversion only ever sees an integer in int16 range (v_cvt_i32_f32 saturates and maps NaN to 0 on its own, C
 * leaves both undefined; v_med3_f32 and fmin / fmax differ from comparisons on NaN).  Contraction is off: there is nothing
 * to contract, and it stays that way. */
#ifndef AAD_PCM_CONVERT_H
#define AAD_PCM_CONVERT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define AAD_PCM_CONVERT_FN __host__ __device__ inline
#else
#define AAD_PCM_CONVERT_FN inline
#endif

namespace aad {

AAD_PCM_CONVERT_FN int32_t pcm_from_f32(float v)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float s = v * 32768.0f;
  if (!(s == s)) return 0; /* NaN, quiet or signalling */
  const float c = s < -32768.0f ? -32768.0f : (s > 32767.0f ? 32767.0f : s);
  return (int32_t)__builtin_rintf(c); /* round to nearest, ties to even (the default mode on both sides) */
}

} /* namespace aad */

#undef AAD_PCM_CONVERT_FN

#endif /* AAD_PCM_CONVERT_H */
