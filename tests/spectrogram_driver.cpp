// spectrogram_driver - aad_amd/csrc/aad_spectrogram.h on the host, for tests/test_spectrogram_host.py and the geometry of
// tests/test_gpu_spectrogram.py: one command per run, arrays through binary files.
//   coefficients <n_fft> <W> <window file: W float32> <out file>   -> "ok <q>" and int16 [W][B][2] in the file, or "refused"
//   planes <n_fft> <W> <cos_sin file> <out file>                   -> "<pairs> <steps> <bytes>"; the planes, then int64 [2][16 pairs]
//   bands <M> <B> <pairs> <filters file: M * B float32> <out file> -> per filter "lo hi offset", then "total <n>", then per pair its
//                                                                     list; the packed weights in the file; or "refused"
//   frames <T> <W> <H>                                             -> "<F>" or "refused"
//   geometry <W> <H>                                               -> "<pitch> <tile_frames> <frame_major> <plane_elements> <lds with filters>"
//   rows <num_rows> <rows> <row_pitch> <frames> <out> <W> <H> <columns> <tile_frames> -> "ok <F> <tiles> <items>" or "refused"
//   shape <n_fft> <W> <H>                                          -> "ok" or "refused"
//   constants                                                      -> "<kSpectrumTileFrames> <kSpectrumThreads> <kSpectrumSpan> <kSpectrumMaxFft>"
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "aad_spectrogram.h"

template <class T>
static std::vector<T> read_file(const char *path, size_t count)
{
  std::vector<T> v(count ? count : 1);
  FILE *f = fopen(path, "rb");
  if (f == nullptr || fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  fclose(f);
  return v;
}

static void write_file(const char *path, const void *p, size_t bytes)
{
  FILE *f = fopen(path, "wb");
  if (f == nullptr || fwrite(p, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot write %s\n", path);
    exit(2);
  }
  fclose(f);
}

int main(int argc, char **argv)
{
  const std::string cmd = argc > 1 ? argv[1] : "";
  const auto u = [&](int i) { return i < argc ? strtoull(argv[i], nullptr, 0) : 0ull; };
  if (cmd == "coefficients" && argc == 6) {
    const uint32_t n_fft = (uint32_t)u(2), W = (uint32_t)u(3);
    const std::vector<float> window = read_file<float>(argv[4], W);
    const size_t n = aad::spectrum_shape_ok(n_fft, W, 1) ? (size_t)W * aad::spectrum_bins(n_fft) * 2 : 0;
    std::vector<int16_t> m(n + 1, (int16_t)0x5A5A);
    uint32_t q = 77;
    if (!aad::spectrum_quantise(window.data(), n_fft, W, m.data(), &q)) {
      bool clean = q == 77;
      for (int16_t v : m) clean = clean && v == (int16_t)0x5A5A;
      printf(clean ? "refused\n" : "refused and wrote\n");
      return 0;
    }
    write_file(argv[5], m.data(), 2 * n);
    printf("ok %u%s\n", q, m[n] == (int16_t)0x5A5A ? "" : " overrun");
  } else if (cmd == "planes" && argc == 6) {
    const uint32_t n_fft = (uint32_t)u(2), W = (uint32_t)u(3), pairs = aad::spectrum_pairs(n_fft);
    const std::vector<int16_t> m = read_file<int16_t>(argv[4], (size_t)W * aad::spectrum_bins(n_fft) * 2);
    const size_t bytes = (size_t)aad::spectrum_plane_bytes(n_fft, W);
    std::vector<int8_t> out(bytes + 8 * 32 * pairs);
    aad::spectrum_build_planes(m.data(), n_fft, W, out.data());
    std::vector<int64_t> consts(32 * pairs);
    aad::spectrum_column_constants(m.data(), n_fft, W, consts.data());
    memcpy(out.data() + bytes, consts.data(), 8 * consts.size());
    write_file(argv[5], out.data(), out.size());
    printf("%u %u %zu\n", pairs, aad::spectrum_steps(W), bytes);
  } else if (cmd == "bands" && argc == 7) {
    const uint32_t M = (uint32_t)u(2), B = (uint32_t)u(3), pairs = (uint32_t)u(4);
    const std::vector<float> filters = read_file<float>(argv[5], (size_t)M * B);
    std::vector<aad::SpectrumBand> bands(M ? M : 1);
    uint64_t total = 0;
    if (!aad::spectrum_bands(filters.data(), M, B, bands.data(), &total)) {
      printf("refused\n");
      return 0;
    }
    std::vector<float> packed(total ? total : 1);
    aad::spectrum_pack_weights(filters.data(), M, B, bands.data(), packed.data());
    write_file(argv[6], packed.data(), 4 * (size_t)total);
    for (uint32_t j = 0; j < M; j++) printf("%u %u %u\n", bands[j].lo, bands[j].hi, bands[j].offset);
    printf("total %llu\n", (unsigned long long)total);
    std::vector<uint32_t> first(pairs + 1);
    aad::spectrum_tile_lists(bands.data(), M, B, pairs, first.data(), nullptr);
    std::vector<uint32_t> list(first[pairs] ? first[pairs] : 1);
    aad::spectrum_tile_lists(bands.data(), M, B, pairs, first.data(), list.data());
    for (uint32_t c = 0; c < pairs; c++) {
      printf("pair");
      for (uint32_t i = first[c]; i < first[c + 1]; i++) printf(" %u", list[i]);
      printf("\n");
    }
  } else if (cmd == "frames") {
    uint32_t F = 77;
    if (aad::spectrum_frames((uint32_t)u(2), (uint32_t)u(3), (uint32_t)u(4), &F)) printf("%u\n", F);
    else printf(F == 77 ? "refused\n" : "refused and wrote\n");
  } else if (cmd == "geometry") {
    const aad::SpectrumGeometry g = aad::spectrum_geometry((uint32_t)u(2), (uint32_t)u(3));
    printf("%u %u %u %u %u\n", g.pitch, g.tile_frames, g.frame_major, g.plane_elements, aad::spectrum_lds_bytes(g, true));
  } else if (cmd == "rows") {
    const aad::SpectrumRows r = aad::spectrum_rows(u(2), u(3), u(4), (uint32_t)u(5), u(6), (uint32_t)u(7), (uint32_t)u(8), (uint32_t)u(9), (uint32_t)u(10));
    if (r.ok) printf("ok %u %u %llu\n", r.num_frames, r.tiles, (unsigned long long)r.items);
    else printf("refused\n");
  } else if (cmd == "shape") {
    printf(aad::spectrum_shape_ok((uint32_t)u(2), (uint32_t)u(3), (uint32_t)u(4)) ? "ok\n" : "refused\n");
  } else if (cmd == "constants") {
    printf("%u %u %u %u\n", aad::kSpectrumTileFrames, aad::kSpectrumThreads, aad::kSpectrumSpan, aad::kSpectrumMaxFft);
  } else {
    printf("unknown\n");
    return 1;
  }
  return 0;
}
