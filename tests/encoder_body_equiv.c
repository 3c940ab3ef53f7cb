/* Exhaustive proof that the quad encoder's fused dequantiser (aad_amd/csrc/aad_encode.hip.h
 * encode_chunk16_quad, region B) equals the reference's (src/aad_encoder.c:384-397):
 *   qd = sign ? -((step * (2 mag + 1)) >> (bits-1)) : (step * (2 mag + 1)) >> (bits-1),  y = clip16(qd + p)
 * The device computes, in one v_mad_i64_i32,
 *   yq = upper dword of  (step << 9) * g + {lo: m, hi: p},   g = ((mag ^ m) << (25 - bits)) | 2^(24 - bits)
 * with m = sign ? -1 : 0, then qd = yq - p and y = clip16(yq).  Checked for every table step, every bit
 * width, every magnitude 0..magmax, both signs and every prediction p in [-65536, 65535] (|sum| < 2^31,
 * so p = sum >> 15 lies there).  The arithmetic below is the instruction's: signed 32 x 32 -> 64-bit
 * product plus a 64-bit addend, upper dword taken as it is. */
#include <stdint.h>
#include <stdio.h>
#include "../aad_amd/csrc/aad_tables_data.h"

static const uint16_t T[256] = {AAD_STEP_TABLE_VALUES};

static int32_t clip16(int32_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

int main(void)
{
  long bad = 0, checked = 0;
  for (int bits = 2; bits <= 4; bits++) {
    const uint32_t magmax = (1u << (bits - 1)) - 1u;
    for (int i = 0; i < 256; i++) {
      const uint32_t step9 = (uint32_t)T[i] << 9; /* the wide record's step << kWideStepShift */
      if (step9 >= (1u << 24)) bad++;             /* the rounding argument needs step << 9 < 2^24 */
      for (uint32_t mag = 0; mag <= magmax; mag++) {
        for (int sign = 0; sign <= 1; sign++) {
          const int32_t m = sign ? -1 : 0;
          int32_t q = (int32_t)((T[i] * ((mag << 1) + 1)) >> (bits - 1));
          const int32_t want_qd = sign ? -q : q;
          const uint32_t g = ((mag ^ (uint32_t)m) << (25 - bits)) | (1u << (24 - bits));
          for (int32_t p = -65536; p <= 65535; p++) {
            const uint64_t mp = (uint64_t)(uint32_t)m | ((uint64_t)(uint32_t)p << 32);
            const uint64_t t = (uint64_t)((int64_t)(int32_t)step9 * (int64_t)(int32_t)g) + mp;
            const int32_t yq = (int32_t)(uint32_t)(t >> 32);
            const int32_t qd = (int32_t)((uint32_t)yq - (uint32_t)p);
            bad += qd != want_qd || clip16(yq) != clip16(want_qd + p);
            checked++;
          }
        }
      }
    }
  }
  printf("%ld %ld\n", checked, bad);
  return bad != 0;
}
