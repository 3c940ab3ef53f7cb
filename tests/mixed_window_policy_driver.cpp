/* Prints aad_launch_policy.h's mixed-format window decode arithmetic for the rows on stdin, one line each
 * (tests/test_mixed_window_policy.py).  A format is four numbers: bits block_size samples_per_block ch_process_method.
 *   V channels n  <n formats>
 *     -> count, then per variant in the helper's order "bits mid_side min_samples_per_block streams"
 *   R channels n  <n formats>
 *     -> per stream its StreamFormat record "samples_per_block block_size bits mid_side"
 *   M cus lds_per_cu decode_lds_pad windows frames channels n  <n formats>
 *     -> ok count, then per launch "bits mid_side min_samples_per_block blocks_per_window workgroup grid lds lanes elements"
 *   K frames samples_per_block
 *     -> window_blocks_spanned */
#include <cstdio>
#include <vector>

#include "aad_launch_policy.h"

static bool read_formats(unsigned channels, unsigned n, std::vector<aad::StreamFormat> *out)
{
  for (unsigned i = 0; i < n; i++) {
    unsigned bits, block_size, spb, method;
    if (scanf("%u %u %u %u", &bits, &block_size, &spb, &method) != 4) return false;
    AADHeaderInfo h = {};
    h.num_channels = (uint16_t)channels;
    h.bits_per_sample = (uint16_t)bits;
    h.block_size = (uint16_t)block_size;
    h.num_samples_per_block = spb;
    h.ch_process_method = (AADChannelProcessMethod)method;
    out->push_back(aad::stream_format_of(h, channels));
  }
  return true;
}

int main()
{
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'V' || kind == 'R') {
      unsigned channels, n;
      std::vector<aad::StreamFormat> f;
      if (scanf("%u %u", &channels, &n) != 2 || !read_formats(channels, n, &f)) return 1;
      if (kind == 'R') {
        for (const aad::StreamFormat &r : f) printf("%u %u %u %u ", r.samples_per_block, (unsigned)r.block_size, (unsigned)r.bits, (unsigned)r.mid_side);
        printf("\n");
        continue;
      }
      const aad::WindowVariants v = aad::window_variants(f.data(), f.size());
      printf("%u", v.count);
      for (unsigned i = 0; i < v.count; i++) printf(" %u %u %u %u", v.v[i].bits, v.v[i].mid_side, v.v[i].min_samples_per_block, v.v[i].streams);
      printf("\n");
    } else if (kind == 'M') {
      aad::Device d;
      aad::Knobs k;
      unsigned long long windows;
      unsigned frames, channels, n;
      std::vector<aad::StreamFormat> f;
      if (scanf("%u %u %d %llu %u %u %u", &d.cus, &d.lds_per_cu, &k.decode_lds_pad, &windows, &frames, &channels, &n) != 7 ||
          !read_formats(channels, n, &f))
        return 1;
      const aad::MixedWindowLaunch m = aad::plan_mixed_window_decode(d, k, aad::window_variants(f.data(), f.size()), windows, frames, channels);
      printf("%d %u", (int)m.ok, m.count);
      for (unsigned i = 0; i < m.count; i++) {
        const aad::WindowLaunch &p = m.launch[i];
        printf(" %u %u %u %u %u %u %u %llu %llu", m.variant[i].bits, m.variant[i].mid_side, m.variant[i].min_samples_per_block,
               p.blocks_per_window, p.workgroup, p.grid, p.lds, (unsigned long long)p.lanes, (unsigned long long)p.elements);
      }
      printf("\n");
    } else if (kind == 'K') {
      unsigned long long frames, spb;
      if (scanf("%llu %llu", &frames, &spb) != 2) return 1;
      printf("%llu\n", (unsigned long long)aad::window_blocks_spanned(frames, spb));
    } else {
      return 1;
    }
  }
  return 0;
}
