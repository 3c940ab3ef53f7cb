// Host driver over aad_amd/csrc/aad_resample.h for tests/test_resample_mix_host.py: the arithmetic the FIR kernels of
// AADHip_ResamplerRunGain / AADHip_ResamplerRunStats run per row - the clip of a span and the row's `count`.  One answer line per
// request line:
//   span  <num_frames> <out_frame> <frames>                      -> Le
//   count <c_src> <source_frames> <shift> <L> <M> <Le>          -> resample_output_count
//   sweep <L> <M> <K> <source_frames>                            -> resample_output_count for c_src in 0 .. K + 40 (outer),
//                                                                   shift in 0 .. K/2 - 1, Le in {0, 1, 7, 300} (inner), one line
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "aad_resample.h"

int main()
{
  char line[256];
  while (fgets(line, sizeof(line), stdin) != nullptr) {
    uint64_t a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
    if (sscanf(line, "span %" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3) {
      printf("%" PRIu64 "\n", aad::resample_span_frames(a, b, (uint32_t)c));
    } else if (sscanf(line, "count %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c, &d, &e, &f) == 6) {
      printf("%" PRIu64 "\n", aad::resample_output_count(a, (uint32_t)b, (uint32_t)c, (uint32_t)d, (uint32_t)e, f));
    } else if (sscanf(line, "sweep %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c, &d) == 4) {
      const uint64_t spans[4] = {0, 1, 7, 300};
      for (uint64_t c_src = 0; c_src <= c + 40; c_src++)
        for (uint64_t shift = 0; shift < c / 2; shift++)
          for (uint64_t le : spans)
            printf("%" PRIu64 " ", aad::resample_output_count(c_src, (uint32_t)d, (uint32_t)shift, (uint32_t)a, (uint32_t)b, le));
      printf("\n");
    } else {
      printf("unknown\n");
    }
  }
  return 0;
}
