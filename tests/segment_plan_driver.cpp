/* Prints aad_segments.h's chain table for the batches on stdin (tests/test_segment_plan.py).
 *   channels spb block_size segment_blocks warmup_blocks num_streams, then per stream: pcm_offset data_offset num_samples
 *     -> "ok <chains>" and one line per chain: pcm_offset data_offset first_block num_frames warmup_blocks header_samples writes_header
 *     -> "refused <chains>" (segment_chain_count) when build_segment_chains refuses the batch */
#include <cstdio>
#include <vector>

#include "aad_segments.h"

int main()
{
  unsigned ch, spb, bs, L, W, n;
  while (scanf("%u %u %u %u %u %u", &ch, &spb, &bs, &L, &W, &n) == 6) {
    std::vector<AADHipStreamDesc> streams(n);
    for (unsigned i = 0; i < n; i++) {
      unsigned long long pcm, data;
      unsigned samples;
      if (scanf("%llu %llu %u", &pcm, &data, &samples) != 3) return 1;
      streams[i] = AADHipStreamDesc{pcm, data, 0, samples, 0};
    }
    std::vector<aad::ChainDesc> t;
    if (!aad::build_segment_chains(streams.data(), n, ch, spb, bs, L, W, &t)) {
      printf("refused %llu\n", L ? (unsigned long long)aad::segment_chain_count(streams.data(), n, spb, L) : 0ull);
      continue;
    }
    printf("ok %zu\n", t.size());
    for (const aad::ChainDesc &c : t)
      printf("%llu %llu %llu %u %u %u %u\n", (unsigned long long)c.pcm_offset, (unsigned long long)c.data_offset,
             (unsigned long long)c.first_block, c.num_frames, c.warmup_blocks, c.header_samples, c.writes_header);
  }
  return 0;
}
