// Host driver of tests/test_planar_stats_host.py: which stream each chain of a segmented plan's chain table belongs to
// (aad_amd/csrc/aad_segments.h chain_streams - the records a statistics run's chains add into), and the kernel argument structs the
// statistics pointer must leave alone.  Reads "spb L W n len..." lines, prints per line the chains' streams.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "aad_segments.h"

int main()
{
  unsigned spb, L, W, n;
  while (scanf("%u %u %u %u", &spb, &L, &W, &n) == 4) {
    std::vector<AADHipStreamDesc> streams(n);
    for (unsigned i = 0; i < n; i++) {
      unsigned len;
      if (scanf("%u", &len) != 1) return 2;
      streams[i] = AADHipStreamDesc{0, 0, 0, len, 0};
    }
    std::vector<aad::ChainDesc> chains;
    if (!aad::build_segment_chains(streams.data(), n, 2, spb, 64, L, W, &chains, true)) return 3;
    for (uint32_t s : aad::chain_streams(chains)) printf("%u ", s);
    printf("\n");
  }
  return 0;
}
