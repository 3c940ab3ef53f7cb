/* Prints aad_segments.h's waves of the host-memory path for the batches on stdin (tests/test_segmented_cli_host.py).
 *   channels spb block_size segment_blocks warmup_blocks budget num_streams, then per stream: num_samples image_size
 *     -> "ok <waves>", per wave "wave <chains> <pcm_elems> <out_begin> <out_bytes>" and one line per chain:
 *        stream frame0 image_offset image_bytes out_offset pcm_offset data_offset first_block num_frames warmup_blocks header_samples
 *        writes_header
 *     -> "refused" when build_segment_waves refuses the batch */
#include <cstdio>
#include <vector>

#include "aad_segments.h"

int main()
{
  unsigned ch, spb, bs, L, W, n;
  unsigned long long budget;
  while (scanf("%u %u %u %u %u %llu %u", &ch, &spb, &bs, &L, &W, &budget, &n) == 7) {
    std::vector<uint32_t> samples(n);
    std::vector<uint64_t> sizes(n);
    for (unsigned i = 0; i < n; i++) {
      unsigned long long size;
      if (scanf("%u %llu", &samples[i], &size) != 2) return 1;
      sizes[i] = size;
    }
    std::vector<aad::SegmentWave> waves;
    if (!aad::build_segment_waves(samples.data(), sizes.data(), n, ch, spb, bs, L, W, budget, &waves)) {
      printf("refused\n");
      continue;
    }
    printf("ok %zu\n", waves.size());
    for (const aad::SegmentWave &t : waves) {
      printf("wave %zu %llu %llu %llu\n", t.chains.size(), (unsigned long long)t.pcm_elems, (unsigned long long)t.out_begin,
             (unsigned long long)t.out_bytes);
      for (size_t k = 0; k < t.chains.size(); k++) {
        const aad::WaveChain &w = t.where[k];
        const aad::ChainDesc &c = t.chains[k];
        printf("%u %u %llu %llu %llu %llu %llu %llu %u %u %u %u\n", w.stream, w.frame0, (unsigned long long)w.image_offset,
               (unsigned long long)w.image_bytes, (unsigned long long)w.out_offset, (unsigned long long)c.pcm_offset,
               (unsigned long long)c.data_offset, (unsigned long long)c.first_block, c.num_frames, c.warmup_blocks, c.header_samples,
               c.writes_header);
      }
    }
  }
  return 0;
}
