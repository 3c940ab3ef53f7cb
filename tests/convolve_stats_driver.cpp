// convolve_stats_driver - aad_amd/csrc/aad_convolve.h's convolve_output_count on the host, for tests/test_convolve_stats_host.py:
// one command per input line, one line of output per command.
//   count <c_src> <source_frames> <shift> <Le>   -> "<count>"
//   sweep <T_src> <S shifts> <L lengths>         -> the counts for c_src = 0 ... T_src + 3, each shift and each Le, in that order
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "aad_convolve.h"

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "count") {
      unsigned long long c_src, source_frames, shift, le;
      in >> c_src >> source_frames >> shift >> le;
      printf("%llu\n", (unsigned long long)aad::convolve_output_count(c_src, (uint32_t)source_frames, (uint32_t)shift, le));
    } else if (cmd == "sweep") {
      unsigned long long t_src, ns, nl;
      in >> t_src >> ns >> nl;
      std::vector<unsigned long long> shifts(ns), lengths(nl);
      for (auto &v : shifts) in >> v;
      for (auto &v : lengths) in >> v;
      for (unsigned long long c = 0; c <= t_src + 3; c++)
        for (unsigned long long shift : shifts)
          for (unsigned long long le : lengths)
            printf("%llu ", (unsigned long long)aad::convolve_output_count(c, (uint32_t)t_src, (uint32_t)shift, le));
      printf("\n");
    } else {
      printf("unknown\n");
    }
  }
  return 0;
}
