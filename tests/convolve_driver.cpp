// convolve_driver - aad_amd/csrc/aad_convolve.h on the host, for tests/test_convolve_host.py: one command per input line, one
// line of output per command.
//   q <delay> <K> <K float32 bit patterns, hex>   -> "ok <q> <delay> <K taps>" or "refused"
//   split                                         -> "ok" when 256 hh + hl == h for every tap in the bound, both in int8, and
//                                                    256 xh + xl + 128 == x for every int16 sample
//   planes <K> <K taps>                           -> "<steps> <bias> <the planes' bytes, hex>"
//   resolve <stream> <first> <response> <R> <R leads> -> "<stream> <src_first> <response> <shift>"
//   source <frames> <max taps>                    -> "<T_src>" or "refused"
//   element <acc> <q>                             -> "<int16> <float32 bits, hex>"
#include <stdio.h>
#include <stdlib.h>

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
    if (cmd == "q") {
      long delay;
      unsigned K;
      in >> delay >> K;
      std::vector<float> h(K ? K : 1);
      for (unsigned k = 0; k < K && k < h.size(); k++) {
        std::string word;
        in >> word;
        const uint32_t bits = (uint32_t)strtoul(word.c_str(), nullptr, 16);
        memcpy(&h[k], &bits, 4);
      }
      std::vector<int16_t> taps(K <= aad::kConvolveMaxTaps ? K + 1 : 1, (int16_t)0x5A5A);
      uint32_t q = 77, d = 77;
      if (!aad::convolve_quantise(h.data(), K, (int32_t)delay, taps.data(), &q, &d)) {
        bool clean = q == 77 && d == 77;
        for (int16_t t : taps) clean = clean && t == (int16_t)0x5A5A;
        printf(clean ? "refused\n" : "refused and wrote\n");
        continue;
      }
      printf("ok %u %u", q, d);
      for (unsigned k = 0; k < K; k++) printf(" %d", taps[k]);
      printf("%s\n", taps[K] == (int16_t)0x5A5A ? "" : " overrun");
    } else if (cmd == "split") {
      bool ok = true;
      for (int h = -aad::kConvolveMaxTap; h <= aad::kConvolveMaxTap; h++) {
        const aad::ConvolveBytes b = aad::convolve_split((int16_t)h);
        ok = ok && 256 * (int)b.hh + (int)b.hl == h;
      }
      for (int x = -32768; x <= 32767; x++) {
        const aad::ConvolveBytes b = aad::convolve_split_sample((int16_t)x);
        ok = ok && 256 * (int)b.hh + (int)b.hl + 128 == x;
      }
      const aad::ConvolveBytes zero = aad::convolve_split_sample(0), low = aad::convolve_split(-128), top = aad::convolve_split(32639);
      ok = ok && zero.hh == 0 && zero.hl == -128 && low.hh == 0 && low.hl == -128 && top.hh == 127 && top.hl == 127;
      printf(ok ? "ok\n" : "wrong\n");
    } else if (cmd == "planes") {
      unsigned K;
      in >> K;
      std::vector<int16_t> taps(K);
      for (unsigned k = 0; k < K; k++) {
        int v;
        in >> v;
        taps[k] = (int16_t)v;
      }
      const uint32_t steps = aad::convolve_steps(K);
      std::vector<int8_t> planes((size_t)steps * aad::kConvolveStepBytes + 16, (int8_t)0x5A);
      aad::convolve_build_planes(taps.data(), K, planes.data());
      printf("%u %lld ", steps, (long long)aad::convolve_bias(taps.data(), K));
      for (int8_t b : planes) printf("%02x", (unsigned)(uint8_t)b);
      printf("\n");
    } else if (cmd == "resolve") {
      unsigned long long stream, first, response;
      unsigned R;
      in >> stream >> first >> response >> R;
      std::vector<uint32_t> lead(R);
      for (unsigned r = 0; r < R; r++) in >> lead[r];
      const aad::ConvolveResolved r = aad::convolve_resolve(stream, first, response, R, lead.data());
      printf("%llu %llu %u %u\n", (unsigned long long)r.stream, (unsigned long long)r.src_first, r.lane.response, r.lane.shift);
    } else if (cmd == "source") {
      unsigned frames, taps;
      in >> frames >> taps;
      uint64_t n = 0;
      if (aad::convolve_source_frames(frames, taps, &n)) printf("%llu\n", (unsigned long long)n);
      else printf("refused\n");
    } else if (cmd == "element") {
      long long acc;
      unsigned q;
      in >> acc >> q;
      const float f = aad::convolve_float(acc, q);
      uint32_t bits;
      memcpy(&bits, &f, 4);
      printf("%d %08x\n", (int)aad::convolve_int16(acc, q), bits);
    } else {
      printf("unknown\n");
    }
  }
  return 0;
}
