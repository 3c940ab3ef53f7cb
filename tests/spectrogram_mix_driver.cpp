// spectrogram_mix_driver - the mix rule of aad_amd/csrc/aad_spectrogram.h on the host, for tests/test_spectrogram_mix_host.py: one
// command per run, arrays through binary files.
//   samples <count> <in file> <out file>   in: per element float32 ga, float32 gb, int16 a, int16 b, int16 inside, int16 unused
//                                          -> "ok"; int16 [count] of spectrum_mix_sample in the out file
//   span <L> <o> <T>                       -> "<Le>"
//   rows <num_rows> <rows_a> <pitch_a> <rows_b> <pitch_b> <rows_per_gain> <gain_a> <gain_b> <spans> <frames> <out> <W> <H> <columns>
//        <tile_frames>                     -> "ok <F> <tiles> <items>" or "refused"
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "aad_spectrogram.h"

struct Element {
  float ga, gb;
  int16_t a, b, inside, unused;
};
static_assert(sizeof(Element) == 16, "the element record");

int main(int argc, char **argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  const auto u = [&](int i) { return i < argc ? strtoull(argv[i], nullptr, 0) : 0ull; };
  if (cmd == "samples" && argc == 5) {
    const size_t count = (size_t)u(2);
    std::vector<Element> in(count ? count : 1);
    FILE *f = fopen(argv[3], "rb");
    if (f == nullptr || fread(in.data(), sizeof(Element), count, f) != count) {
      fprintf(stderr, "cannot read %s\n", argv[3]);
      return 2;
    }
    fclose(f);
    std::vector<int16_t> out(count ? count : 1);
    for (size_t i = 0; i < count; i++) out[i] = aad::spectrum_mix_sample(in[i].ga, in[i].a, in[i].gb, in[i].b, in[i].inside != 0);
    f = fopen(argv[4], "wb");
    if (f == nullptr || fwrite(out.data(), sizeof(int16_t), count, f) != count) {
      fprintf(stderr, "cannot write %s\n", argv[4]);
      return 2;
    }
    fclose(f);
    printf("ok\n");
  } else if (cmd == "span" && argc == 5) {
    printf("%u\n", aad::spectrum_mix_span(u(2), u(3), (uint32_t)u(4)));
  } else if (cmd == "rows" && argc == 17) {
    const aad::SpectrumRows r = aad::spectrum_mix_rows(u(2), u(3), u(4), u(5), u(6), (uint32_t)u(7), u(8), u(9), u(10), (uint32_t)u(11), u(12),
                                                       (uint32_t)u(13), (uint32_t)u(14), (uint32_t)u(15), (uint32_t)u(16));
    if (r.ok) printf("ok %u %u %llu\n", r.num_frames, r.tiles, (unsigned long long)r.items);
    else printf("refused\n");
  } else {
    printf("unknown\n");
    return 1;
  }
  return 0;
}
