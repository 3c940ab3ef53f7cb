/* Prints aad_launch_policy.h's channel-mix window decode arithmetic for the rows on stdin, one line each
 * (tests/test_channel_mix_policy.py).  A format is five numbers: channels bits block_size samples_per_block ch_process_method.
 *   V n  <n formats>
 *     -> count, then per variant in the helper's order "channels bits mid_side min_samples_per_block streams"
 *   R n  <n formats>
 *     -> per stream its ChannelStreamFormat record "samples_per_block block_size bits source"
 *   M cus lds_per_cu decode_lds_pad windows frames out_channels n  <n formats>
 *     -> ok count, then per launch "channels bits mid_side min_samples_per_block blocks_per_window workgroup grid lds lanes elements" */
#include <cstdio>
#include <vector>

#include "aad_launch_policy.h"

static bool read_formats(unsigned n, std::vector<aad::ChannelStreamFormat> *out)
{
  for (unsigned i = 0; i < n; i++) {
    unsigned channels, bits, block_size, spb, method;
    if (scanf("%u %u %u %u %u", &channels, &bits, &block_size, &spb, &method) != 5) return false;
    AADHeaderInfo h = {};
    h.num_channels = (uint16_t)channels;
    h.bits_per_sample = (uint16_t)bits;
    h.block_size = (uint16_t)block_size;
    h.num_samples_per_block = spb;
    h.ch_process_method = (AADChannelProcessMethod)method;
    out->push_back(aad::channel_stream_format_of(h));
  }
  return true;
}

int main()
{
  char kind;
  while (scanf(" %c", &kind) == 1) {
    if (kind == 'V' || kind == 'R') {
      unsigned n;
      std::vector<aad::ChannelStreamFormat> f;
      if (scanf("%u", &n) != 1 || !read_formats(n, &f)) return 1;
      if (kind == 'R') {
        for (const aad::ChannelStreamFormat &r : f)
          printf("%u %u %u %u ", r.samples_per_block, (unsigned)r.block_size, (unsigned)r.bits, (unsigned)r.source);
        printf("\n");
        continue;
      }
      const aad::ChannelMixVariants v = aad::channel_mix_variants(f.data(), f.size());
      printf("%u", v.count);
      for (unsigned i = 0; i < v.count; i++)
        printf(" %u %u %u %u %u", v.v[i].channels, v.v[i].bits, v.v[i].mid_side, v.v[i].min_samples_per_block, v.v[i].streams);
      printf("\n");
    } else if (kind == 'M') {
      aad::Device d;
      aad::Knobs k;
      unsigned long long windows;
      unsigned frames, out_channels, n;
      std::vector<aad::ChannelStreamFormat> f;
      if (scanf("%u %u %d %llu %u %u %u", &d.cus, &d.lds_per_cu, &k.decode_lds_pad, &windows, &frames, &out_channels, &n) != 7 ||
          !read_formats(n, &f))
        return 1;
      const aad::ChannelMixWindowLaunch m =
          aad::plan_channel_mix_window_decode(d, k, aad::channel_mix_variants(f.data(), f.size()), windows, frames, out_channels);
      printf("%d %u", (int)m.ok, m.count);
      for (unsigned i = 0; i < m.count; i++) {
        const aad::WindowLaunch &p = m.launch[i];
        printf(" %u %u %u %u %u %u %u %u %llu %llu", m.variant[i].channels, m.variant[i].bits, m.variant[i].mid_side,
               m.variant[i].min_samples_per_block, p.blocks_per_window, p.workgroup, p.grid, p.lds, (unsigned long long)p.lanes,
               (unsigned long long)p.elements);
      }
      printf("\n");
    } else {
      return 1;
    }
  }
  return 0;
}
