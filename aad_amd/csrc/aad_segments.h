/* aad_segments.h - the chain table of a segmented encode plan (AADHip_SegmentedEncodePlanCreate), host-only C++17 apart from the
 * record itself, which the encoder kernel reads, so that a CPU test pins it (tests/test_segment_plan.py).
 *
 * A stream of N frames, spb samples per block, B = ceil(N / spb) blocks, is cut into segments of L blocks: segment s keeps blocks
 * [s L, min((s + 1) L, B)).  Its chain is a fresh encoder over frames [(s L - w) spb, min((s + 1) L spb, N)), w = min(W, s L): the
 * first w blocks are warm-up (encoded, then discarded), the rest are the segment's bytes at their place in the stream's image.
 * Every block header carries the decoder's whole state, so the image is a valid stream whatever chain wrote a block. */
#ifndef AAD_SEGMENTS_H
#define AAD_SEGMENTS_H

#include <stdint.h>

#include <vector>

#include "../../include/aad_hip.h"

namespace aad {

/* one chain of a segmented encode: one segment of one stream, all of its channels */
struct ChainDesc {
  uint64_t pcm_offset;     /* index of the int16 that starts the chain's first encoded frame (a warm-up frame, if any) */
  uint64_t data_offset;    /* byte offset of the STREAM's image */
  uint64_t first_block;    /* index in the stream of the chain's first encoded block (the first warm-up block, if any) */
  uint32_t num_frames;     /* frames the chain encodes, warm-up included */
  uint32_t warmup_blocks;  /* blocks encoded before the first kept one and not stored */
  uint32_t header_samples; /* the stream's num_samples, for the file header */
  uint32_t writes_header;  /* 1: the chain keeps block 0 and writes the 31-byte file header */
};
static_assert(sizeof(ChainDesc) == 40, "ChainDesc is uploaded as is");

inline uint64_t stream_blocks(uint32_t num_samples, uint32_t spb) { return ((uint64_t)num_samples + spb - 1) / spb; }

/* chains of a batch: ceil(B / L) per stream (one for a stream of less than a block) */
inline uint64_t segment_chain_count(const AADHipStreamDesc *streams, uint32_t num_streams, uint32_t spb, uint32_t segment_blocks)
{
  uint64_t n = 0;
  for (uint32_t i = 0; i < num_streams; i++) {
    const uint64_t b = stream_blocks(streams[i].num_samples, spb);
    n += b == 0 ? 1u : (b + segment_blocks - 1) / segment_blocks;
  }
  return n;
}

/* The chain table of a batch, stream by stream and segment by segment.  False (and `out` untouched) when a geometry term is zero
 * or the batch has more than UINT32_MAX chains (the kernel indexes chains with 32 bits).  block_size only bounds the table: a
 * chain's blocks lie at 31 + block * block_size in its stream's image, which the 64-bit offsets hold for any stream. */
inline bool build_segment_chains(const AADHipStreamDesc *streams, uint32_t num_streams, uint32_t channels, uint32_t spb,
                                 uint32_t block_size, uint32_t segment_blocks, uint32_t warmup_blocks, std::vector<ChainDesc> *out)
{
  if (channels == 0 || spb == 0 || block_size == 0 || segment_blocks == 0) return false;
  const uint64_t count = segment_chain_count(streams, num_streams, spb, segment_blocks);
  if (count > UINT32_MAX) return false;
  std::vector<ChainDesc> t;
  t.reserve((size_t)count);
  const uint64_t L = segment_blocks;
  for (uint32_t i = 0; i < num_streams; i++) {
    const AADHipStreamDesc &sd = streams[i];
    const uint64_t n = sd.num_samples, b = stream_blocks(sd.num_samples, spb);
    const uint64_t segments = b == 0 ? 1u : (b + L - 1) / L;
    for (uint64_t s = 0; s < segments; s++) {
      const uint64_t kept = s * L, w = warmup_blocks < kept ? warmup_blocks : kept;
      const uint64_t first_frame = (kept - w) * spb, end_frame = (s + 1) * L * spb < n ? (s + 1) * L * spb : n;
      ChainDesc c;
      c.pcm_offset = sd.pcm_offset + first_frame * channels;
      c.data_offset = sd.data_offset;
      c.first_block = kept - w;
      c.num_frames = (uint32_t)(end_frame - first_frame);
      c.warmup_blocks = (uint32_t)w;
      c.header_samples = sd.num_samples;
      c.writes_header = s == 0 ? 1u : 0u;
      t.push_back(c);
    }
  }
  out->swap(t);
  return true;
}

} /* namespace aad */

#endif /* AAD_SEGMENTS_H */
