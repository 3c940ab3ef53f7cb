/* Host driver of the planar encode's CPU tests (tests/test_planar_host.py), built with g++ against the device code's own headers.
 *   exhaustive              -> "mismatches <count> <first bit pattern, hex>": aad_pcm_convert.h's pcm_from_f32 against q_plain over
 *                              all 2^32 float32 bit patterns
 *   convert <in> <out>      -> pcm_from_f32 of every float32 in file <in> (little endian) as int32 to file <out>
 *   chains <planar: 0 | 1>  -> aad_segments.h's chain table for the batches on stdin, in tests/segment_plan_driver.cpp's format */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "aad_pcm_convert.h"
#include "aad_segments.h"

/* q as include/aad_hip.h states it, in plain C on doubles: v * 32768 is exact there, the tie rule is spelled out */
static int32_t q_plain(float v)
{
  if (std::isnan(v)) return 0;
  const double s = (double)v * 32768.0;
  if (s <= -32768.0) return -32768;
  if (s >= 32767.0) return 32767;
  const double f = std::floor(s), r = s - f;
  long long k = (long long)f;
  if (r > 0.5 || (r == 0.5 && (k & 1))) k++;
  return (int32_t)k;
}

static int exhaustive()
{
  unsigned threads = std::thread::hardware_concurrency();
  threads = threads < 1 ? 1 : (threads > 16 ? 16 : threads);
  std::vector<unsigned long long> bad(threads, 0), first(threads, ~0ull);
  std::vector<std::thread> pool;
  const unsigned long long total = 1ull << 32, per = (total + threads - 1) / threads;
  for (unsigned t = 0; t < threads; t++)
    pool.emplace_back([&, t]() {
      const unsigned long long lo = t * per, hi = lo + per < total ? lo + per : total;
      for (unsigned long long b = lo; b < hi; b++) {
        const uint32_t bits = (uint32_t)b;
        float v;
        std::memcpy(&v, &bits, 4);
        if (aad::pcm_from_f32(v) != q_plain(v)) {
          if (bad[t] == 0) first[t] = b;
          bad[t]++;
        }
      }
    });
  for (std::thread &th : pool) th.join();
  unsigned long long n = 0, f = ~0ull;
  for (unsigned t = 0; t < threads; t++) {
    n += bad[t];
    if (first[t] < f) f = first[t];
  }
  printf("mismatches %llu %llx\n", n, n ? f : 0ull);
  return 0;
}

static int convert(const char *in, const char *out)
{
  FILE *f = fopen(in, "rb");
  if (!f) return 1;
  std::vector<float> x;
  float v;
  while (fread(&v, 4, 1, f) == 1) x.push_back(v);
  fclose(f);
  std::vector<int32_t> y(x.size());
  for (size_t i = 0; i < x.size(); i++) y[i] = aad::pcm_from_f32(x[i]);
  f = fopen(out, "wb");
  if (!f) return 1;
  const bool ok = fwrite(y.data(), 4, y.size(), f) == y.size();
  fclose(f);
  return ok ? 0 : 1;
}

static int chains(bool planar)
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
    if (!aad::build_segment_chains(streams.data(), n, ch, spb, bs, L, W, &t, planar)) {
      printf("refused\n");
      continue;
    }
    printf("ok %zu\n", t.size());
    for (const aad::ChainDesc &c : t)
      printf("%llu %llu %llu %u %u %u %u\n", (unsigned long long)c.pcm_offset, (unsigned long long)c.data_offset,
             (unsigned long long)c.first_block, c.num_frames, c.warmup_blocks, c.header_samples, c.writes_header);
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 2 && !strcmp(argv[1], "exhaustive")) return exhaustive();
  if (argc == 4 && !strcmp(argv[1], "convert")) return convert(argv[2], argv[3]);
  if (argc == 3 && !strcmp(argv[1], "chains")) return chains(atoi(argv[2]) != 0);
  fprintf(stderr, "usage: exhaustive | convert <in> <out> | chains <planar>\n");
  return 2;
}
