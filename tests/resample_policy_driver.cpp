/* resample_policy_driver.cpp - runs aad_amd/csrc/aad_resample.h on the CPU for tests/test_resample_host.py.  One command per line
 * of standard input, one line of output each:
 *   ratio UP DOWN            -> "refused zero" | "refused shape L M K" | "refused sum L M K S" | "ok L M K S", S the largest sum |h|
 *   bank UP DOWN             -> "L M K" and then the L * K coefficients, phase by phase, on the same line (an accepted ratio)
 *   frames T L M K           -> "refused" | T_src
 *   resolve STREAM FIRST VARIANT  over the table of `table`  -> "stream src_first bank shift"
 *   table NUM_STREAMS VARIANTS NUM_BANKS  and then NUM_STREAMS * VARIANTS select entries and NUM_BANKS leads -> "ok"
 * TEST INFRASTRUCTURE (tests/ only). */
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aad_resample.h"

int main()
{
  char cmd[32];
  std::vector<uint16_t> select, lead;
  uint64_t num_streams = 0;
  uint32_t variants = 1;
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "ratio") || !strcmp(cmd, "bank")) {
      uint32_t up, down;
      if (scanf("%" SCNu32 " %" SCNu32, &up, &down) != 2) return 2;
      aad::ResampleRatio r;
      if (!aad::resample_reduce(up, down, &r)) {
        printf("refused zero\n");
        continue;
      }
      const uint64_t K = aad::resample_taps(r.L, r.M);
      if (!aad::resample_shape_ok(r.L, r.M)) {
        printf("refused shape %u %u %" PRIu64 "\n", r.L, r.M, K);
        continue;
      }
      std::vector<int16_t> h((size_t)r.L * K);
      const bool ok = aad::resample_build_bank(r.L, r.M, h.data());
      if (!strcmp(cmd, "ratio")) {
        uint32_t most = 0; /* the largest sum |h| of a phase */
        for (uint32_t p = 0; p < r.L; p++) {
          uint32_t sum = 0;
          for (uint64_t k = 0; k < K; k++) sum += (uint32_t)(h[p * K + k] < 0 ? -h[p * K + k] : h[p * K + k]);
          most = sum > most ? sum : most;
        }
        printf("%s %u %u %" PRIu64 " %u\n", ok ? "ok" : "refused sum", r.L, r.M, K, most);
        continue;
      }
      if (!ok) return 3;
      printf("%u %u %" PRIu64, r.L, r.M, K);
      for (int16_t v : h) printf(" %d", v);
      printf("\n");
    } else if (!strcmp(cmd, "frames")) {
      uint32_t t, L, M, K;
      if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &t, &L, &M, &K) != 4) return 2;
      uint64_t n = 0;
      if (aad::resample_source_frames(t, L, M, K, &n)) printf("%" PRIu64 "\n", n);
      else printf("refused\n");
    } else if (!strcmp(cmd, "table")) {
      uint32_t banks;
      if (scanf("%" SCNu64 " %" SCNu32 " %" SCNu32, &num_streams, &variants, &banks) != 3) return 2;
      select.assign((size_t)num_streams * variants, 0);
      lead.assign(banks, 0);
      for (uint16_t &v : select)
        if (scanf("%" SCNu16, &v) != 1) return 2;
      for (uint16_t &v : lead)
        if (scanf("%" SCNu16, &v) != 1) return 2;
      printf("ok\n");
    } else if (!strcmp(cmd, "resolve")) {
      uint64_t stream, first, variant;
      if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &stream, &first, &variant) != 3) return 2;
      const aad::ResampleResolved r = aad::resample_resolve(stream, first, variant, num_streams, variants, select.data(), lead.data());
      printf("%" PRIu64 " %" PRIu64 " %u %u\n", r.stream, r.src_first, r.lane.bank, r.lane.shift);
    } else {
      return 2;
    }
  }
  return 0;
}
