/* Exhaustive proof that the quad mapping's fused LMS tap update (aad_amd/csrc/aad_device.hip.h lms_first_fused) equals the
 * reference's (src/aad_encoder.c:396-400, src/aad_decoder.c:306-310):
 *   w += (qd * h + 16384) >> 18        in int32
 * The device computes, in one v_mad_i64_i32,
 *   w' = upper dword of  q14 * h + {lo: 2^28, hi: w},   q14 = qd << 14
 * Part 1: for every qd in [-65536, 65535] and every int16 h (2^33 pairs) the upper dword of q14 * h + 2^28 is the
 * reference's increment.  The reference's own int32 expression overflows for exactly one of those pairs,
 * qd = -65536 and h = -32768 (the product is 2^31: undefined in C, -8192 where it wraps); there the device form gives the
 * exact value, +8192, and the program checks that and that it is the only such pair.  No encoder or decoder gets there:
 * |qd| <= (32767 * 15) >> 3 = 61438, the largest table step at the largest 4-bit magnitude (checked below against the table).
 * Part 2: for the weights in the file argv[1] (one decimal int32 per line) the full form equals the wrapped sum, over a grid
 * of qd and h that holds both rails of each, zero, +-1 and +-61438.
 * The arithmetic below is the instruction's: signed 32 x 32 -> 64-bit product plus a 64-bit addend, upper dword taken as it is.
 * Output: pairs checked, mismatches, pairs where the reference overflows, (weight, qd, h) triples checked, mismatches. */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include "../aad_amd/csrc/aad_tables_data.h"

static const uint16_t T[256] = {AAD_STEP_TABLE_VALUES};

static int32_t fused_increment(int32_t qd, int32_t h)
{
  const int32_t q14 = (int32_t)((uint32_t)qd << 14);
  return (int32_t)(uint32_t)((uint64_t)((int64_t)q14 * (int64_t)h + (int64_t)(1ll << 28)) >> 32);
}
static int32_t fused_update(int32_t w, int32_t qd, int32_t h)
{
  const int32_t q14 = (int32_t)((uint32_t)qd << 14);
  const uint64_t addend = ((uint64_t)(uint32_t)w << 32) | (1u << 28);
  return (int32_t)(uint32_t)((uint64_t)((int64_t)q14 * (int64_t)h + (int64_t)addend) >> 32);
}
/* the reference's increment; *overflow: its int32 expression leaves int32 */
static int32_t reference_increment(int32_t qd, int32_t h, int *overflow)
{
  const int64_t exact = (int64_t)qd * (int64_t)h + 16384;
  *overflow = exact > INT32_MAX || exact < INT32_MIN;
  return (int32_t)((int32_t)(uint32_t)(uint64_t)exact >> 18); /* the wrapped value where it overflows */
}

struct Slice {
  int32_t qd_lo, qd_hi; /* [lo, hi) */
  long checked, bad, overflowed;
};

static void *run_slice(void *arg)
{
  struct Slice *s = (struct Slice *)arg;
  for (int32_t qd = s->qd_lo; qd < s->qd_hi; qd++) {
    long bad = 0;
    for (int32_t h = -32768; h <= 32767; h++) { /* no overflow inside: |qd * h| < 2^31 but for the pair below */
      const int32_t want = (int32_t)((uint32_t)qd * (uint32_t)h + 16384u) >> 18;
      bad += fused_increment(qd, h) != want;
    }
    s->checked += 65536;
    if (qd == -65536) { /* the reference's overflow: look at h = -32768 by itself */
      int ovf;
      const int32_t wrapped = reference_increment(qd, -32768, &ovf);
      if (ovf && wrapped == -8192 && fused_increment(qd, -32768) == 8192) {
        s->overflowed++;
        bad--; /* counted as a mismatch by the loop above */
      }
    }
    s->bad += bad;
  }
  return NULL;
}

int main(int argc, char **argv)
{
  long bad_table = 0;
  for (int i = 0; i < 256; i++) bad_table += ((T[i] * 15) >> 3) > 61438 || T[i] > 32767;

  long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
  int threads = ncpu < 1 ? 1 : ncpu > 16 ? 16 : (int)ncpu;
  pthread_t tid[16];
  struct Slice sl[16];
  for (int t = 0; t < threads; t++) {
    sl[t].qd_lo = -65536 + (int32_t)((131072ll * t) / threads);
    sl[t].qd_hi = -65536 + (int32_t)((131072ll * (t + 1)) / threads);
    sl[t].checked = sl[t].bad = sl[t].overflowed = 0;
    if (pthread_create(&tid[t], NULL, run_slice, &sl[t])) return 2;
  }
  long checked = 0, bad = bad_table, overflowed = 0;
  for (int t = 0; t < threads; t++) {
    pthread_join(tid[t], NULL);
    checked += sl[t].checked;
    bad += sl[t].bad;
    overflowed += sl[t].overflowed;
  }
  /* every other pair's reference value is free of overflow: |qd * h| + 16384 <= 65536 * 32767 + 16384 < 2^31 */

  long wchecked = 0, wbad = 0;
  if (argc > 1) {
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    static int32_t qds[600], hs[600];
    int nq = 0, nh = 0;
    const int32_t qx[] = {-65536, 65535, -61438, 61438, 0, 1, -1};
    const int32_t hx[] = {-32768, 32767, 0, 1, -1};
    for (unsigned i = 0; i < sizeof qx / sizeof *qx; i++) qds[nq++] = qx[i];
    for (int32_t q = -65536 + 3; q <= 65535; q += 509) qds[nq++] = q;
    for (unsigned i = 0; i < sizeof hx / sizeof *hx; i++) hs[nh++] = hx[i];
    for (int32_t h = -32768 + 5; h <= 32767; h += 127) hs[nh++] = h;
    long long v;
    while (fscanf(f, "%lld", &v) == 1) {
      const int32_t w = (int32_t)v;
      for (int a = 0; a < nq; a++)
        for (int b = 0; b < nh; b++) {
          int ovf;
          const int32_t inc = reference_increment(qds[a], hs[b], &ovf);
          if (ovf) continue; /* the one pair of part 1 */
          wbad += fused_update(w, qds[a], hs[b]) != (int32_t)((uint32_t)w + (uint32_t)inc);
          wchecked++;
        }
    }
    fclose(f);
  }
  printf("%ld %ld %ld %ld %ld\n", checked, bad, overflowed, wchecked, wbad);
  return bad != 0 || wbad != 0;
}
