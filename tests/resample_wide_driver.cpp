/* resample_wide_driver.cpp - runs what aad_amd/csrc/aad_resample.h says about a wide resampler (AADHip_ResamplerCreateWide) on
 * the CPU for tests/test_resample_wide_host.py.  One command per line of standard input, one line of output each:
 *   shape UP DOWN     -> "refused zero" | "refused L M K" | "ok L M K RESIDENT PLAIN": the limits alone, no bank is built;
 *                        RESIDENT: resample_bank_resident, PLAIN: resample_shape_ok (what AADHip_ResamplerCreate accepts)
 *   bank UP DOWN      -> "L M K" and then the L * K coefficients of the library's builder, phase by phase, on the same line
 *   plan L M K        -> "R ROWS INDEX SPAN": resample_gather_round(K) and resample_gather_lds at that R, in bytes
 *   gather L M R TILE T  -> "ok OUTPUTS ROUNDS" | "bad ..."; walks tile TILE of a row of T outputs as the gathered kernel does: 256
 *                        threads, thread tid's outputs TILE * 1024 + tid + 256 j with (i, p) stepped by (256 M) div / mod L, each
 *                        published at resample_gather_slot's row of its round - and then holds every output n of the tile to
 *                        index[row] == (n M) mod L and i == (n M) div L, the rows of a round to R consecutive outputs, no row
 *                        written twice
 * TEST INFRASTRUCTURE (tests/ only). */
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "aad_resample.h"

int main()
{
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "shape") || !strcmp(cmd, "bank")) {
      uint32_t up, down;
      if (scanf("%" SCNu32 " %" SCNu32, &up, &down) != 2) return 2;
      aad::ResampleRatio r;
      if (!aad::resample_reduce(up, down, &r)) {
        printf("refused zero\n");
        continue;
      }
      const uint64_t K = aad::resample_taps(r.L, r.M);
      if (!aad::resample_wide_shape_ok(r.L, r.M)) {
        printf("refused %u %u %" PRIu64 "\n", r.L, r.M, K);
        continue;
      }
      if (!strcmp(cmd, "shape")) {
        printf("ok %u %u %" PRIu64 " %d %d\n", r.L, r.M, K, (int)aad::resample_bank_resident(r.L, (uint32_t)K),
               (int)aad::resample_shape_ok(r.L, r.M));
        continue;
      }
      std::vector<int16_t> h((size_t)r.L * K);
      if (!aad::resample_build_bank(r.L, r.M, h.data())) return 3;
      printf("%u %u %" PRIu64, r.L, r.M, K);
      for (int16_t v : h) printf(" %d", v);
      printf("\n");
    } else if (!strcmp(cmd, "plan")) {
      uint32_t L, M, K;
      if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &L, &M, &K) != 3) return 2;
      const uint32_t R = aad::resample_gather_round(K);
      const aad::ResampleGatherLds lds = aad::resample_gather_lds(L, M, K, R);
      printf("%u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", R, lds.rows, lds.index, lds.span);
    } else if (!strcmp(cmd, "gather")) {
      uint32_t L, M, R, tile, T;
      if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &L, &M, &R, &tile, &T) != 5) return 2;
      const uint32_t threads = aad::kResampleThreads, n0 = tile * aad::kResampleTile;
      const uint32_t n_end = T - n0 < aad::kResampleTile ? T : n0 + aad::kResampleTile;
      const uint32_t rounds = (aad::kResampleTile + R - 1) / R;
      std::vector<std::vector<int64_t>> index(rounds, std::vector<int64_t>(R, -1)), owner(rounds, std::vector<int64_t>(R, -1));
      const uint32_t step = threads * M, di = step / L, dp = step - di * L;
      const char *bad = nullptr;
      uint64_t outputs = 0;
      for (uint32_t tid = 0; tid < threads; tid++) {
        uint32_t n = n0 + tid;
        const uint32_t nm = n * M;
        uint32_t i = nm / L, p = nm - i * L;
        for (uint32_t j = 0; j < aad::kResamplePerThread; j++, n += threads) {
          const aad::ResampleGatherSlot slot = aad::resample_gather_slot(j * threads + tid, R);
          if (n < n_end) {
            if (slot.round >= rounds || slot.row >= R) bad = "slot out of range";
            else if (index[slot.round][slot.row] != -1) bad = "row written twice";
            else {
              index[slot.round][slot.row] = p;
              owner[slot.round][slot.row] = n;
              if ((uint64_t)i != (uint64_t)n * M / L) bad = "source frame";
              outputs++;
            }
          }
          i += di;
          p += dp;
          if (p >= L) {
            p -= L;
            i += 1;
          }
        }
      }
      uint32_t used = 0;
      for (uint32_t r = 0; r < rounds && bad == nullptr; r++)
        for (uint32_t t = 0; t < R; t++) {
          const uint64_t n = (uint64_t)n0 + (uint64_t)r * R + t; /* a round is R consecutive outputs */
          if (n >= n_end) {
            if (index[r][t] != -1) bad = "row past the end";
            continue;
          }
          if (t == 0) used++;
          if (owner[r][t] != (int64_t)n) bad = "rows of a round are not consecutive outputs";
          else if (index[r][t] != (int64_t)(n * M % L)) bad = "phase";
        }
      if (bad == nullptr && outputs != n_end - n0) bad = "outputs missing";
      if (bad != nullptr) printf("bad %s\n", bad);
      else printf("ok %" PRIu64 " %u\n", outputs, used);
    } else {
      return 2;
    }
  }
  return 0;
}
