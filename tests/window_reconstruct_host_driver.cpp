/* Host driver of the window reconstruct's CPU tests (tests/test_window_reconstruct_host.py), built with g++ against the header the
 * resolve kernel itself is compiled from (aad_amd/csrc/aad_windows.h) and the host builders of aad_segments.h.
 *   lanes   -> for each line "<spb> <L> <W> <T> <image_stride> <stream_stride> <src_offset> <w> <S> <stream> <first_frame> <n_0> ..."
 *              on stdin (L 0: unsegmented): "<len_w> <lanes per window> <real lanes> <verdict>", verdict being "same" when every
 *              lane window_lane gives equals what build_segment_chains + reconstruct_output_bases + chain_streams give for a single
 *              stream of len_w frames at src_offset + first_frame placed as stream w, and every lane behind those has
 *              num_frames == 0, warmup_blocks == 0 and writes_header == 0; else the first difference
 *   refuse  -> for each line on stdin "ok" or "refused":
 *                "images <N> <image_stride> <image_bytes>"             window_images_ok
 *                "lanes <N> <T> <spb> <L>"                             window_lane_count
 *                "rows <C> <N> <T> <type> <reserved> <ss> <cs>"        planar_output_rows_ok
 *                "sources <C> <cs> <elem_bytes> <S> <offset> <n> ..."  window_sources_ok */
#include <cstdio>
#include <cstring>
#include <vector>

#include "aad_launch_policy.h"
#include "aad_segments.h"
#include "aad_windows.h"

typedef unsigned long long ull;

static int lanes()
{
  unsigned spb, L, W, T, S;
  ull image_stride, ss, src, w, stream, first;
  while (scanf("%u %u %u %u %llu %llu %llu %llu %u %llu %llu", &spb, &L, &W, &T, &image_stride, &ss, &src, &w, &S, &stream, &first) == 11) {
    std::vector<AADHipStreamDesc> sources(S);
    for (unsigned i = 0; i < S; i++) {
      unsigned n;
      if (scanf("%u", &n) != 1) return 1;
      sources[i] = AADHipStreamDesc{src + 1000ull * i, 0, 0, n, 0};
    }
    const uint32_t len = aad::window_length(stream, first, T, S, sources.data());
    aad::WindowGeometry g;
    memset(&g, 0, sizeof(g));
    g.frames = T;
    g.spb = spb;
    g.segment_blocks = L;
    g.warmup_blocks = W;
    g.chains_per_window = (uint32_t)aad::window_chains(T, spb, L);
    g.image_stride = image_stride;
    g.out_stream_stride = ss;
    /* the host's plan for the one stream the window is */
    const AADHipStreamDesc crop = {len != 0 ? sources[stream].pcm_offset + first : 0, w * image_stride, 0, len, 0};
    std::vector<aad::ChainDesc> chains;
    if (L != 0 && !aad::build_segment_chains(&crop, 1, 2, spb, 64, L, W, &chains, true)) return 1;
    const std::vector<uint64_t> base = aad::reconstruct_output_bases(1, ss, L != 0 ? &chains : nullptr, spb);
    const std::vector<uint32_t> of = aad::chain_streams(chains);
    const size_t real = L != 0 ? chains.size() : 1;
    const char *verdict = "same";
    if (real > g.chains_per_window) verdict = "more chains than the uniform launch has lanes";
    for (uint32_t k = 0; k < g.chains_per_window && !strcmp(verdict, "same"); k++) {
      const aad::WindowLane r = aad::window_lane(g, w, k, len != 0 ? sources[stream].pcm_offset : 12345, first, len);
      if (r.data_offset != w * image_stride || r.stats_stream != (uint32_t)w) verdict = "image or statistics row";
      else if (k >= real) {
        if (r.num_frames != 0 || r.writes_header != 0 || r.warmup_blocks != 0) verdict = "padding lane is not empty";
      } else if (L == 0) {
        if (r.pcm_offset != crop.pcm_offset || r.num_frames != crop.num_samples || r.out_base != w * ss + base[0] || r.writes_header != 1)
          verdict = "stream lane";
      } else {
        const aad::ChainDesc &c = chains[k];
        if (r.pcm_offset != c.pcm_offset) verdict = "pcm_offset";
        else if (r.first_block != c.first_block) verdict = "first_block";
        else if (r.num_frames != c.num_frames) verdict = "num_frames";
        else if (r.warmup_blocks != c.warmup_blocks) verdict = "warmup_blocks";
        else if (r.header_samples != c.header_samples) verdict = "header_samples";
        else if (r.writes_header != c.writes_header) verdict = "writes_header";
        else if (r.out_base != w * ss + base[k]) verdict = "out_base";
        else if (of[k] != 0) verdict = "chain_streams";
      }
    }
    printf("%u %u %zu %s\n", len, g.chains_per_window, real, verdict);
  }
  return 0;
}

static int refuse()
{
  char what[16];
  while (scanf("%15s", what) == 1) {
    bool ok = false;
    if (!strcmp(what, "images")) {
      ull n, stride, bytes;
      if (scanf("%llu %llu %llu", &n, &stride, &bytes) != 3) return 1;
      ok = aad::window_images_ok(n, stride, bytes);
    } else if (!strcmp(what, "lanes")) {
      ull n;
      unsigned T, spb, L;
      if (scanf("%llu %u %u %u", &n, &T, &spb, &L) != 4) return 1;
      uint64_t count = 0;
      ok = aad::window_lane_count(n, T, spb, L, &count);
    } else if (!strcmp(what, "rows")) {
      unsigned C, T, reserved;
      int type;
      ull n, ss, cs;
      if (scanf("%u %llu %u %d %u %llu %llu", &C, &n, &T, &type, &reserved, &ss, &cs) != 7) return 1;
      const AADHipPlanarOutput o = {type, reserved, ss, cs};
      ok = aad::planar_output_rows_ok(C, n, T, &o);
    } else if (!strcmp(what, "sources")) {
      unsigned C, elem, S;
      ull cs;
      if (scanf("%u %llu %u %u", &C, &cs, &elem, &S) != 4) return 1;
      std::vector<AADHipStreamDesc> sources(S);
      for (unsigned i = 0; i < S; i++) {
        ull off;
        unsigned n;
        if (scanf("%llu %u", &off, &n) != 2) return 1;
        sources[i] = AADHipStreamDesc{off, 0, 0, n, 0};
      }
      ok = aad::window_sources_ok(C, cs, elem, S, sources.data());
    } else {
      return 1;
    }
    printf("%s\n", ok ? "ok" : "refused");
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 2 && !strcmp(argv[1], "lanes")) return lanes();
  if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
  fprintf(stderr, "usage: lanes | refuse\n");
  return 2;
}
