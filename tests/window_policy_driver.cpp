/* Prints aad_launch_policy.h's window decode arithmetic for the rows on stdin, one line each (tests/test_window_policy.py).
 *   W cus lds_per_cu decode_lds_pad windows frames channels bits samples_per_block
 *     -> ok blocks_per_window workgroup grid lds lanes elements
 *   S frames samples_per_block
 *     -> window_blocks_spanned, then window_blocks_at for every phase 0 .. samples_per_block - 1
 *   L
 *     -> kLdsBytesDenseDec (the static LDS the dense decoders and the window kernel hold) */
#include <cstdio>

#include "aad_launch_policy.h"

int main()
{
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'W') {
      aad::Device d;
      aad::Knobs k;
      aad::WindowBatch b;
      unsigned long long windows;
      if (scanf("%u %u %d %llu %u %u %u %u", &d.cus, &d.lds_per_cu, &k.decode_lds_pad, &windows, &b.frames, &b.channels, &b.bits,
                &b.samples_per_block) != 8)
        return 1;
      b.windows = windows;
      const aad::WindowLaunch p = aad::plan_window_decode(d, k, b);
      printf("%d %u %u %u %u %llu %llu\n", (int)p.ok, p.blocks_per_window, p.workgroup, p.grid, p.lds, (unsigned long long)p.lanes,
             (unsigned long long)p.elements);
    } else if (kind == 'S') {
      unsigned long long frames, spb;
      if (scanf("%llu %llu", &frames, &spb) != 2) return 1;
      printf("%llu", (unsigned long long)aad::window_blocks_spanned(frames, spb));
      for (unsigned long long ph = 0; ph < spb; ph++) printf(" %llu", (unsigned long long)aad::window_blocks_at(ph, frames, spb));
      printf("\n");
    } else if (kind == 'L') {
      printf("%d\n", (int)aad::kLdsBytesDenseDec);
    } else {
      return 1;
    }
  }
  return 0;
}
