/* Host driver of the planar reconstruct's CPU tests (tests/test_planar_reconstruct_host.py), built with g++ against the launch
 * policy header the engine itself plans with.
 *   policy  -> "<batches> <reconstruct QuadDual> <reconstruct DenseRing> <encode QuadDual> <encode DenseRing>": how often
 *              plan_reconstruct_encode and plan_encode pick the dual trial search and the byte ring over a sweep of batches,
 *              lane mappings and trial-lane / ring settings
 *   output  -> for each line "<channels> <type> <reserved> <stream_stride> <channel_stride> <n> <num_samples> ..." on stdin:
 *              "ok" or "refused" from planar_output_ok
 *   bases   -> for each line "<spb> <segment_blocks> <warmup_blocks> <stream_stride> <n> <num_samples> ..." on stdin: the plan's
 *              per-lane output bases (reconstruct_output_bases over the chain table of build_segment_chains; segment_blocks 0: an
 *              unsegmented plan, one lane per stream), space-separated on one line */
#include <cstdio>
#include <cstring>
#include <vector>

#include "aad_launch_policy.h"
#include "aad_segments.h"

static int policy()
{
  const aad::Device d = {256, 160 * 1024};
  unsigned long long batches = 0, rec_dual = 0, rec_ring = 0, enc_dual = 0, enc_ring = 0;
  const uint32_t mappings[] = {AAD_HIP_LANE_MAPPING_AUTO, AAD_HIP_LANE_MAPPING_DENSE, AAD_HIP_LANE_MAPPING_QUAD, AAD_HIP_LANE_MAPPING_QUAD_FUSED};
  const uint32_t streams[] = {1, 40, 1000, 2560, 4096, 5000, 16384, 40000, 65536, 262144, 1000000};
  for (uint32_t m : mappings)
    for (int32_t lanes = 0; lanes < 2; lanes++)
      for (int32_t ring = 0; ring < 3; ring++)
        for (uint32_t bits = 2; bits <= 4; bits++)
          for (uint32_t ch = 1; ch <= 3; ch++)
            for (uint32_t trials : {0u, 1u, 2u, 5u})
              for (uint32_t n : streams)
                for (int ring_ok = 0; ring_ok < 2; ring_ok++) {
                  aad::Knobs k;
                  k.lane_mapping = (int32_t)m;
                  k.trial_lanes = lanes ? AAD_HIP_TRIAL_LANES_SINGLE : AAD_HIP_TRIAL_LANES_DUAL;
                  k.encode_ring = ring;
                  const aad::EncodeBatch b = {bits, ch, n, trials, 1024, ring_ok != 0};
                  const aad::EncodeLaunch r = aad::plan_reconstruct_encode(d, k, b), e = aad::plan_encode(d, k, b);
                  batches++;
                  rec_dual += r.kernel == aad::EncodeKernel::QuadDual || r.trial_scratch_bytes != 0;
                  rec_ring += r.kernel == aad::EncodeKernel::DenseRing;
                  enc_dual += e.kernel == aad::EncodeKernel::QuadDual;
                  enc_ring += e.kernel == aad::EncodeKernel::DenseRing;
                }
  printf("%llu %llu %llu %llu %llu\n", batches, rec_dual, rec_ring, enc_dual, enc_ring);
  return 0;
}

static int output()
{
  unsigned ch, n;
  int type;
  unsigned reserved;
  unsigned long long ss, cs;
  while (scanf("%u %d %u %llu %llu %u", &ch, &type, &reserved, &ss, &cs, &n) == 6) {
    std::vector<AADHipStreamDesc> streams(n);
    for (unsigned i = 0; i < n; i++) {
      unsigned samples;
      if (scanf("%u", &samples) != 1) return 1;
      streams[i] = AADHipStreamDesc{0, 0, 0, samples, 0};
    }
    const AADHipPlanarOutput o = {type, reserved, ss, cs};
    printf("%s\n", aad::planar_output_ok(ch, n, streams.data(), &o) ? "ok" : "refused");
  }
  return 0;
}

static int bases()
{
  unsigned spb, L, W, n;
  unsigned long long ss;
  while (scanf("%u %u %u %llu %u", &spb, &L, &W, &ss, &n) == 5) {
    std::vector<AADHipStreamDesc> streams(n);
    for (unsigned i = 0; i < n; i++) {
      unsigned samples;
      if (scanf("%u", &samples) != 1) return 1;
      streams[i] = AADHipStreamDesc{0, 0, 0, samples, 0};
    }
    std::vector<aad::ChainDesc> chains;
    if (L != 0 && !aad::build_segment_chains(streams.data(), n, 2, spb, 64, L, W, &chains, true)) return 1;
    for (uint64_t b : aad::reconstruct_output_bases(n, ss, L != 0 ? &chains : nullptr, spb)) printf("%llu ", (unsigned long long)b);
    printf("\n");
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 2 && !strcmp(argv[1], "policy")) return policy();
  if (argc == 2 && !strcmp(argv[1], "output")) return output();
  if (argc == 2 && !strcmp(argv[1], "bases")) return bases();
  fprintf(stderr, "usage: policy | output | bases\n");
  return 2;
}
