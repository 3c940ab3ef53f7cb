/* window_span_driver.cpp - runs aad_amd/csrc/aad_window_span.h, the arithmetic window_lane's PLACED mode runs on the device, on the
 * host (tests/test_window_placed_host.py).  One line in per case: T spb spb_min phase L o; one line out:
 *   Le K bad max_tile crop_elements fill_elements
 * K = window_blocks_spanned(T, spb_min), the lanes a window has when the launch is planned from spb_min <= spb.  The driver walks
 * the K lanes as the kernel does - a lane's crop range [lo, hi) shifted to the row by o unless the lane is `past` or the span is
 * empty, and its two fill pieces - and counts, element by element, how often each element of [0, T) is owned.  bad: the number
 * of elements not owned exactly once, plus one for every piece that reaches outside [0, T), every crop element outside
 * [o, o + Le) and every fill element inside it.  max_tile: the most elements any lane fills.
 * TEST INFRASTRUCTURE (tests/ only). */
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "aad_launch_policy.h"
#include "aad_window_span.h"

int main()
{
  unsigned long long T, spb, spb_min, phase, L, o;
  while (scanf("%llu %llu %llu %llu %llu %llu", &T, &spb, &spb_min, &phase, &L, &o) == 6) {
    const uint64_t le = aad::window_span_frames(L, o, (uint32_t)T);
    const uint64_t K = aad::window_blocks_spanned(T, spb_min);
    std::vector<int> owners(T, 0);
    uint64_t bad = 0, max_tile = 0, crop_elements = 0, fill_elements = 0;
    auto own = [&](int64_t t, bool crop) {
      if (t < 0 || t >= (int64_t)T) {
        bad++;
        return;
      }
      const bool inside = le != 0 && (uint64_t)t >= o && (uint64_t)t < o + le;
      if (inside != crop) bad++;
      owners[(size_t)t]++;
      (crop ? crop_elements : fill_elements)++;
    };
    for (uint32_t k = 0; k < K; k++) {
      const aad::WindowFillTile tile = aad::window_fill_tile(k, spb, phase, (uint32_t)T, o, le);
      uint64_t filled = 0;
      for (int j = 0; j < 2; j++)
        for (int64_t t = tile.lo[j]; t < tile.hi[j]; t++, filled++) own(t, false);
      if (filled > max_tile) max_tile = filled;
      if (le == 0) continue;
      const aad::WindowCropRange r = aad::window_crop_range(k, spb, phase, le);
      if (r.past) continue;
      for (int64_t i = r.lo; i < r.hi; i++) own((int64_t)o + i, true);
    }
    for (uint64_t t = 0; t < T; t++) bad += owners[t] != 1;
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", le, K, bad, max_tile, crop_elements,
           fill_elements);
  }
  return 0;
}
