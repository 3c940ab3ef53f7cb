/* Prints aad_launch_policy.h's plans for the batches on stdin, one line each (tests/test_launch_policy.py).
 *   E cus lds_per_cu | mapping trial_lanes encode_ring encode_lds_pad decode_lds_pad decode_nt_min | bits channels streams trials block_size ring_ok
 *     -> kernel trials workgroup grid lds trial_slot_bytes trial_scratch_bytes
 *   R (an E row's fields): the same batch under plan_reconstruct_encode (planar and window reconstruct runs) -> as E
 *   D cus lds_per_cu | (knobs as above) | blocks streams channels bits samples_per_block block_size pcm_aligned16 pcm_base_aligned16
 *     code_phase_uniform stream_stores
 *     -> kernel stream_stores workgroup grid lds residual_bytes residual_stride */
#include <cstdio>

#include "aad_launch_policy.h"

int main()
{
  static const char *const kEncode[] = {"dense", "dense-ring", "quad", "quad-dual"};
  static const char *const kDecode[] = {"split-lds", "split-scratch", "quad-fused", "tiled", "dense"};
  char kind;
  while (scanf(" %c", &kind) == 1) {
    aad::Device d;
    aad::Knobs k;
    unsigned long long nt_min;
    if (scanf("%u %u %d %d %d %d %d %llu", &d.cus, &d.lds_per_cu, &k.lane_mapping, &k.trial_lanes, &k.encode_ring, &k.encode_lds_pad,
              &k.decode_lds_pad, &nt_min) != 8)
      return 1;
    k.decode_nt_min = nt_min;
    if (kind == 'E' || kind == 'R') {
      aad::EncodeBatch b;
      unsigned ring_ok;
      if (scanf("%u %u %u %u %u %u", &b.bits, &b.channels, &b.streams, &b.trials, &b.block_size, &ring_ok) != 6) return 1;
      b.ring_ok = ring_ok != 0;
      const aad::EncodeLaunch p = kind == 'R' ? aad::plan_reconstruct_encode(d, k, b) : aad::plan_encode(d, k, b);
      printf("%s %d %u %u %u %u %llu\n", kEncode[(int)p.kernel], (int)p.trials, p.workgroup, p.grid, p.lds, p.trial_slot_bytes,
             (unsigned long long)p.trial_scratch_bytes);
    } else {
      aad::DecodeBatch b;
      unsigned long long blocks;
      unsigned al16, base_al16, stream_stores;
      if (scanf("%llu %u %u %u %u %u %u %u %u %u", &blocks, &b.streams, &b.channels, &b.bits, &b.samples_per_block, &b.block_size, &al16,
                &base_al16, &b.code_phase_uniform, &stream_stores) != 10)
        return 1;
      b.blocks = blocks;
      b.pcm_aligned16 = al16 != 0;
      b.pcm_base_aligned16 = base_al16 != 0;
      b.stream_stores = stream_stores != 0;
      const aad::DecodeLaunch p = aad::plan_decode(d, k, b);
      printf("%s %d %u %u %u %llu %u\n", kDecode[(int)p.kernel], (int)p.stream_stores, p.workgroup, p.grid, p.lds,
             (unsigned long long)p.residual_bytes, p.residual_stride);
    }
  }
  return 0;
}
