// fir_stage_driver - aad_amd/csrc/aad_fir_stage.h on the host, for tests/test_fir_stage_host.py: one command per input line, one
// line of output per command.
//   tiles                                                           -> "<kResampleTile> <kConvolveTile>"
//   rows <windows> <channels> <frames> <source frames> <needed> <elem> <src> <lanes> <out> <out optional> <tile>
//                                                                   -> "ok <rows> <tiles>" or "refused"
//   resolve <windows> <windows table> <selector> <source windows> <lanes> -> "ok" or "refused"
//   gain <sample type> <mode> <gain> <spans>                        -> "ok" or "refused"
// Addresses and counts are decimal.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "aad_convolve.h"
#include "aad_fir_stage.h"
#include "aad_resample.h"

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "tiles") {
      printf("%u %u\n", aad::kResampleTile, aad::kConvolveTile);
    } else if (cmd == "rows") {
      unsigned long long windows, elem, src, lanes, out;
      unsigned channels, frames, source_frames, needed, out_optional, tile;
      in >> windows >> channels >> frames >> source_frames >> needed >> elem >> src >> lanes >> out >> out_optional >> tile;
      const aad::FirRows f = aad::fir_rows(windows, channels, frames, source_frames, needed, elem, src, lanes, out, out_optional != 0, tile);
      if (f.ok) printf("ok %llu %u\n", (unsigned long long)f.rows, f.tiles);
      else printf("refused\n");
    } else if (cmd == "resolve") {
      unsigned long long windows, table, selector, source_windows, lanes;
      in >> windows >> table >> selector >> source_windows >> lanes;
      printf(aad::fir_resolve_ok(windows, table, selector, source_windows, lanes) ? "ok\n" : "refused\n");
    } else if (cmd == "gain") {
      int sample_type, mode;
      unsigned long long gain, spans;
      in >> sample_type >> mode >> gain >> spans;
      printf(aad::fir_gain_ok(sample_type, mode, gain, spans) ? "ok\n" : "refused\n");
    } else {
      printf("unknown\n");
    }
  }
  return 0;
}
