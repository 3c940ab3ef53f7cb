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
#include "aad_windows.h" /* the segment rule: segment_count, segment_cut */

namespace aad {

/* one chain of a segmented encode: one segment of one stream, all of its channels */
struct ChainDesc {
  uint64_t pcm_offset;     /* index of the int16 that starts the chain's first encoded frame (a warm-up frame, if any); planar input:
                            * of the element that starts channel 0's row there */
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
  for (uint32_t i = 0; i < num_streams; i++) n += segment_count(streams[i].num_samples, spb, segment_blocks);
  return n;
}

/* The chain table of a batch, stream by stream and segment by segment.  False (and `out` untouched) when a geometry term is zero
 * or the batch has more than UINT32_MAX chains (the kernel indexes chains with 32 bits).  block_size only bounds the table: a
 * chain's blocks lie at 31 + block * block_size in its stream's image, which the 64-bit offsets hold for any stream.
 * planar: the streams' PCM is one row per channel (AADHip_PlanarEncodePlanCreate) - a chain starts first_frame elements into
 * channel 0's row, not first_frame frames of interleaved samples into the stream. */
inline bool build_segment_chains(const AADHipStreamDesc *streams, uint32_t num_streams, uint32_t channels, uint32_t spb,
                                 uint32_t block_size, uint32_t segment_blocks, uint32_t warmup_blocks, std::vector<ChainDesc> *out,
                                 bool planar = false)
{
  if (channels == 0 || spb == 0 || block_size == 0 || segment_blocks == 0) return false;
  const uint64_t count = segment_chain_count(streams, num_streams, spb, segment_blocks);
  if (count > UINT32_MAX) return false;
  std::vector<ChainDesc> t;
  t.reserve((size_t)count);
  for (uint32_t i = 0; i < num_streams; i++) {
    const AADHipStreamDesc &sd = streams[i];
    const uint64_t segments = segment_count(sd.num_samples, spb, segment_blocks);
    for (uint64_t s = 0; s < segments; s++) {
      const SegmentCut cut = segment_cut(sd.num_samples, spb, segment_blocks, warmup_blocks, s);
      ChainDesc c;
      c.pcm_offset = sd.pcm_offset + cut.first_frame * (planar ? 1u : channels);
      c.data_offset = sd.data_offset;
      c.first_block = cut.first_block;
      c.num_frames = (uint32_t)(cut.end_frame - cut.first_frame);
      c.warmup_blocks = cut.warmup_blocks;
      c.header_samples = sd.num_samples;
      c.writes_header = s == 0 ? 1u : 0u;
      t.push_back(c);
    }
  }
  out->swap(t);
  return true;
}

/* Where the lanes of a planar reconstruct plan (AADHip_PlanarReconstructPlanCreate) start in its output: per lane the element that
 * holds channel 0's sample of the lane's first frame, stream i's rows starting stream_stride * i elements in.  chains == null: the
 * lanes are the streams.  Else they are the table's chains, and the table's own records say where each starts, as for the waves
 * below: a chain's stream (its one writes_header chain opens it) and its first frame (first_block, the first warm-up block if any). */
inline std::vector<uint64_t> reconstruct_output_bases(uint32_t num_streams, uint64_t stream_stride, const std::vector<ChainDesc> *chains,
                                                      uint32_t spb)
{
  std::vector<uint64_t> base;
  if (chains == nullptr) {
    for (uint32_t i = 0; i < num_streams; i++) base.push_back((uint64_t)i * stream_stride);
    return base;
  }
  uint64_t stream = 0;
  for (size_t c = 0; c < chains->size(); c++) {
    const ChainDesc &d = (*chains)[c];
    if (d.writes_header && c != 0) stream++;
    base.push_back(stream * stream_stride + d.first_block * spb);
  }
  return base;
}

/* per chain of a table the index of its stream, by the same rule (the statistics of a segmented planar reconstruct run: the
 * chains of a stream add into that stream's records) */
inline std::vector<uint32_t> chain_streams(const std::vector<ChainDesc> &chains)
{
  std::vector<uint32_t> of;
  uint32_t stream = 0;
  for (size_t c = 0; c < chains.size(); c++) {
    if (chains[c].writes_header && c != 0) stream++;
    of.push_back(stream);
  }
  return of;
}

/* ---- waves of the host-memory path (AADHip_SegmentedEncodeBatch) ----------------------------------------------------------------
 *
 * A wave is a run of consecutive chains of the batch's chain table that is resident on the device at once and encoded by ONE launch,
 * so that all its chains run side by side: each chain's frames, warm-up included, in the wave's PCM block, and the bytes it keeps in
 * the wave's output block, one chain after the other.  The budget is the device memory a wave may take; only the staging between
 * the caller's buffers and those blocks is cut into chunks.  Chains carry no state, so a wave may end between any two chains; a
 * chain whose input and output alone exceed the budget is a wave of its own.
 *
 * Addressing.  The kernel stores a chain's kept block i at data_offset + 31 + (first_block + w + i) block_size and the file header
 * at data_offset (writes_header only), w being its warm-up.  A wave's table sets first_block = 0 and points data_offset at a VIRTUAL
 * image start `lead` = 31 + w block_size bytes in front of the chain's kept bytes (0 for the header chain, which keeps block 0).
 * Those lead bytes overlap the previous chain's bytes or the block's lead-in and are never written: warm-up blocks store nothing.
 * The lead-in (out_begin) is as large as it must be for every data_offset to be a plain, non-negative offset. */
struct WaveChain {
  uint32_t stream;       /* the chain's stream in the batch */
  uint32_t frame0;       /* first frame of the stream that the chain encodes (its first warm-up frame, if any) */
  uint64_t image_offset; /* first byte of the stream's image that the chain writes: 0 (file header), or 31 + kept block * block_size */
  uint64_t image_bytes;  /* bytes it writes there: up to its last kept block's end, the stream's short last block included */
  uint64_t out_offset;   /* where those bytes lie in the wave's output block */
};

struct SegmentWave {
  std::vector<ChainDesc> chains; /* the launch's chain table: pcm_offset into the wave's PCM block, data_offset into its output block */
  std::vector<WaveChain> where;  /* per chain: its stream, its frames, the bytes it delivers */
  uint64_t pcm_elems = 0;        /* int16 in the PCM block (every chain's frames start on 16 bytes) */
  uint64_t out_begin = 0;        /* the output block's lead-in: its kept bytes are [out_begin, out_bytes) */
  uint64_t out_bytes = 0;
};

inline uint64_t round_up16(uint64_t v) { return (v + 15) / 16 * 16; }

/* The waves of a batch of host streams: num_samples[i] frames, an image of image_size[i] bytes (AADFormat_EncodedSize).  budget:
 * bytes of PCM in + bytes out per wave.  False (and `out` untouched) as build_segment_chains. */
inline bool build_segment_waves(const uint32_t *num_samples, const uint64_t *image_size, uint32_t num_streams, uint32_t channels,
                                uint32_t spb, uint32_t block_size, uint32_t segment_blocks, uint32_t warmup_blocks, uint64_t budget,
                                std::vector<SegmentWave> *out)
{
  std::vector<AADHipStreamDesc> streams(num_streams);
  for (uint32_t i = 0; i < num_streams; i++) streams[i] = AADHipStreamDesc{0, 0, 0, num_samples[i], 0};
  std::vector<ChainDesc> all;
  if (!build_segment_chains(streams.data(), num_streams, channels, spb, block_size, segment_blocks, warmup_blocks, &all)) return false;
  std::vector<SegmentWave> waves;
  SegmentWave t;
  uint64_t cost = 0, pos = 0; /* pos: the chains' bytes so far, from the lead-in's end */
  auto close = [&]() {
    if (t.chains.empty()) return;
    uint64_t lead_in = 0;
    for (size_t k = 0; k < t.chains.size(); k++) {
      const uint64_t lead = t.chains[k].data_offset; /* still the chain's lead, at this point */
      if (lead > t.where[k].out_offset && lead - t.where[k].out_offset > lead_in) lead_in = lead - t.where[k].out_offset;
    }
    t.out_begin = round_up16(lead_in);
    for (size_t k = 0; k < t.chains.size(); k++) {
      t.where[k].out_offset += t.out_begin;
      t.chains[k].data_offset = t.where[k].out_offset - t.chains[k].data_offset;
    }
    t.out_bytes = t.out_begin + pos;
    waves.push_back(std::move(t));
    t = SegmentWave();
    cost = pos = 0;
  };
  /* The table's own records say where a stream starts (its one writes_header chain, the first of its chains) and ends (the next
   * stream's start, or the table's end): nothing here depends on how build_segment_chains counts a stream's segments. */
  uint32_t stream = 0;
  for (size_t c = 0; c < all.size(); c++) {
    const ChainDesc &d = all[c];
    if (d.writes_header && c != 0) stream++;
    if (stream >= num_streams) return false; /* a table that does not match the batch: refused, never misread */
    const bool last = c + 1 == all.size() || all[c + 1].writes_header;
    const uint64_t kept = d.first_block + d.warmup_blocks;
    const uint64_t begin = d.writes_header ? 0 : AAD_HEADER_SIZE + kept * block_size;
    const uint64_t end = last ? image_size[stream] : AAD_HEADER_SIZE + (kept + segment_blocks) * block_size;
    const uint64_t elems = ((uint64_t)d.num_frames * channels + 7) / 8 * 8, bytes = end - begin;
    const uint64_t chain_cost = elems * sizeof(int16_t) + round_up16(bytes);
    if (!t.chains.empty() && cost + chain_cost > budget) close();
    ChainDesc e = d;
    e.pcm_offset = t.pcm_elems;
    e.data_offset = d.writes_header ? 0 : AAD_HEADER_SIZE + (uint64_t)d.warmup_blocks * block_size; /* the lead, made an offset by close() */
    e.first_block = 0;
    t.chains.push_back(e);
    t.where.push_back(WaveChain{stream, (uint32_t)(d.pcm_offset / channels), begin, bytes, pos});
    t.pcm_elems += elems;
    pos += round_up16(bytes);
    cost += chain_cost;
  }
  if (num_streams != 0 && stream + 1 != num_streams) return false;
  close();
  out->swap(waves);
  return true;
}

} /* namespace aad */

#endif /* AAD_SEGMENTS_H */
