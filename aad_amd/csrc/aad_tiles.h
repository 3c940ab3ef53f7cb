/* aad_tiles.h - which bytes of a host-memory batch go where (AADHip_EncodeBatch, AADHip_DecodeBatch, the legacy whole-file calls and
 * aad_batch): how the batch is cut into tiles and what each tile's two pinned blocks hold.  Host-only C++17, no HIP, so that a CPU
 * test pins it (tests/test_host_tiles.py); the pipeline that moves the blocks is run_tiles in aad_hip_engine.hip.
 *
 * How a batch is cut.  A stream's blocks are chained in the encoder (block k starts from the predictor block k-1 left behind), so
 * one launch costs about `blocks per stream` x 64 us however few streams it holds: cutting a batch of long streams BY STREAM would
 * pay that chain once per cut.  The batch is therefore cut both ways: consecutive streams form a GROUP until one block of each
 * fills the tile budget, and a group is walked in TILES of `budget / (streams alive x block bytes)` blocks of every stream at once,
 * the predictor state staying on the device between tiles (encode; decode blocks are independent and only share the tiling).
 * Inside a group streams are ordered longest first, so that the streams still alive at any block are a prefix of that order and a
 * stream's state record keeps its index for the whole group. */
#ifndef AAD_TILES_H
#define AAD_TILES_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/aad_hip.h"
#include "aad_format.h" /* AAD_BLOCK_HEADER_BYTES_PER_CH */

namespace aad {

inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

constexpr uint64_t kChunkBudget = 16ull << 20; /* payload bytes (in + out) per tile of a cut batch */
constexpr uint64_t kCutAbove = kChunkBudget;

/* tile_bytes: AAD_HIP_OPTION_TILE_KBYTES in bytes (forced: tests, tuning), 0 = the built-in budget */
inline bool batch_is_cut(int64_t tile_bytes, uint64_t total_bytes) { return tile_bytes > 0 || total_bytes > kCutAbove; }

inline uint64_t tile_budget(int64_t tile_bytes, uint64_t total_bytes)
{
  if (tile_bytes > 0) return (uint64_t)tile_bytes;
  return total_bytes > kCutAbove ? kChunkBudget : ~0ull >> 8;
}

/* A batch that travels as ONE tile has nothing to overlap with, so its big copy is cut into pieces instead: encode sends piece p
 * up while the host fills piece p + 1, decode drains piece p while piece p + 1 comes down.  Item index where each piece ends, by
 * running bytes (`prefix`: count + 1 entries). */
constexpr uint32_t kMaxPieces = 4;
constexpr uint64_t kPieceBytes = 1ull << 20;

inline uint32_t cut_pieces(const std::vector<uint64_t> &prefix, uint32_t count, bool wanted, uint32_t *end)
{
  const uint64_t total = prefix[count];
  uint32_t pieces = wanted ? (uint32_t)(total / kPieceBytes) : 1u;
  pieces = pieces < 1 ? 1 : (pieces > kMaxPieces ? kMaxPieces : pieces);
  uint32_t at = 0, made = 0;
  for (uint32_t p = 1; p < pieces; p++) {
    const uint64_t target = total / pieces * p;
    while (at < count && prefix[at] < target) at++;
    if (at > (made ? end[made - 1] : 0u) && at < count) end[made++] = at;
  }
  end[made++] = count;
  return made;
}

/* items [*a, *b) whose rows meet bytes [lo, hi) of a block; `at`: count + 1 entries, where each item's row starts and the block ends */
inline void row_span(const std::vector<uint64_t> &at, uint64_t lo, uint64_t hi, uint32_t *a, uint32_t *b)
{
  const uint32_t count = (uint32_t)at.size() - 1;
  *a = (uint32_t)(std::upper_bound(at.begin(), at.end(), lo) - at.begin());
  *a = *a ? *a - 1 : 0;
  *b = (uint32_t)(std::lower_bound(at.begin(), at.end(), hi) - at.begin());
  if (*b > count) *b = count;
}

struct TileStep {
  uint32_t alive;          /* streams in the tile: order[0 .. alive) */
  uint64_t block0, block1; /* blocks [block0, block1) of each */
  bool group_first, group_last;
};

struct TilePlanner {
  const uint64_t *blocks; /* per stream: blocks to walk (0 = nothing to do) */
  uint32_t n;
  uint64_t block_cost, budget;
  uint32_t next_stream = 0;
  bool in_group = false;
  uint64_t block0 = 0;
  std::vector<uint32_t> order; /* the current group, longest stream first */

  TilePlanner(const uint64_t *blocks_per_stream, uint32_t num_streams, uint64_t bytes_per_block, uint64_t tile_budget)
      : blocks(blocks_per_stream), n(num_streams), block_cost(bytes_per_block ? bytes_per_block : 1), budget(tile_budget) {}

  bool next(TileStep *t)
  {
    for (;;) {
      bool first = false;
      if (!in_group) {
        if (next_stream >= n) return false;
        order.clear();
        uint64_t cost = 0;
        do {
          order.push_back(next_stream);
          if (blocks[next_stream]) cost += block_cost;
          next_stream++;
        } while (next_stream < n && cost < budget);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return blocks[x] > blocks[y]; });
        block0 = 0;
        in_group = true;
        first = true;
      }
      /* streams with more than block0 blocks: a prefix of the order */
      uint32_t lo = 0, hi = (uint32_t)order.size();
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (blocks[order[mid]] > block0) lo = mid + 1; else hi = mid;
      }
      if (lo == 0) { /* a group of empty streams */
        in_group = false;
        continue;
      }
      const uint64_t longest = blocks[order[0]];
      uint64_t per_tile = budget / ((uint64_t)lo * block_cost);
      if (per_tile == 0) per_tile = 1;
      t->alive = lo;
      t->block0 = block0;
      t->block1 = longest - block0 <= per_tile ? longest : block0 + per_tile;
      t->group_first = first;
      t->group_last = t->block1 >= longest;
      block0 = t->block1;
      if (t->group_last) in_group = false;
      return true;
    }
  }
};

/* ---- what a tile's two pinned blocks hold ------------------------------------------------------------------------------------
 *
 * A tile is one input block {stream table | block prefix or lane states | payload}, one launch and one output block
 * {payload | lane states}.  Row k of either payload belongs to stream order[k] of the planner's group; rows start on 16 bytes.
 * The layouts below are all the arithmetic between a TileStep and the copies: offsets into the blocks and into the caller's
 * buffers, never pointers. */
struct TileLayout {
  TileStep step;
  std::vector<AADHipStreamDesc> table;         /* the launch's stream table: offsets into the two payloads */
  std::vector<uint64_t> fill_cost, drain_cost; /* [alive + 1]: where row k starts in the input / output payload, in bytes, and its end */
  uint64_t pcm_elems, data_bytes;              /* int16 elements of the PCM payload, bytes of the image payload */
  uint64_t table_bytes, payload_off, in_bytes; /* input block: the table's room, where the payload starts, all of it */
  uint64_t out_bytes, down_bytes;              /* output block: all of it, and what the copy behind the launch brings down */

  void start(const TileStep &s)
  {
    step = s;
    table.resize(s.alive);
    fill_cost.resize((size_t)s.alive + 1);
    drain_cost.resize((size_t)s.alive + 1);
    pcm_elems = data_bytes = 0;
  }
};

/* what the host still has to do with an encoded tile: bytes [src, src + bytes) of the output block are bytes [dst, ...) of
 * stream `stream`'s image */
struct ImageSlice {
  uint32_t stream;
  uint64_t src, dst, bytes;
  bool patch_count; /* the slice opens a longer stream: the file header it carries holds the tile's sample count, and bytes 14..17
                     * of the image take the whole stream's (big-endian) */
};

/* States live on the device while a group has tiles to go; the caller's come in with the first tile and leave with the last.
 *   lone        the group's only tile: states travel inside its blocks
 *   carry       the launch leaves the states in the context's device records, one per channel of the group's group_size streams
 *   state_in    the input block brings the caller's states: row k's stream's at table_bytes + k * channels records
 *   state_back  the output block takes the group's states home: bytes [data_bytes, out_bytes), stream state_order[slot]'s in `slot` */
struct EncodeTile : TileLayout {
  static constexpr bool kCutUp = true; /* a lone tile's input copy is the one cut into pieces */
  std::vector<ImageSlice> items;
  std::vector<uint32_t> state_order; /* state_back: the group as the planner orders it, else empty */
  uint32_t lead, group_size;         /* the trial search looks one block back in the input: later tiles bring that block along */
  uint64_t fill_frame0;              /* every row holds its stream's frames [fill_frame0, fill_frame0 + table[k].num_samples) */
  bool lone, carry, state_in, state_back;
};

/* order: the planner's current group; num_samples / sizes (AADFormat_EncodedSize) / blocks: per stream of the batch */
inline void encode_tile_layout(const TileStep &step, const std::vector<uint32_t> &order, const uint32_t *num_samples, const uint64_t *sizes,
                               const uint64_t *blocks, uint32_t ch, uint32_t spb, uint32_t block_size, bool trials, bool has_state, EncodeTile *t)
{
  const uint32_t n = step.alive;
  t->start(step);
  t->items.resize(n);
  t->group_size = (uint32_t)order.size();
  t->lead = trials && step.block0 > 0 ? spb : 0;
  t->fill_frame0 = step.block0 * spb - t->lead;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t i = order[k];
    const uint64_t frame0 = step.block0 * spb;
    const uint64_t frame1 = step.block1 * spb < num_samples[i] ? step.block1 * spb : num_samples[i];
    /* file header + this tile's blocks: up to the stream's end, or whole blocks */
    const uint64_t slice = AAD_HEADER_SIZE + (step.block1 >= blocks[i] ? sizes[i] - AAD_HEADER_SIZE - step.block0 * block_size
                                                                       : (step.block1 - step.block0) * block_size);
    const uint32_t frames = (uint32_t)(frame1 - frame0) + t->lead;
    t->table[k] = AADHipStreamDesc{t->pcm_elems, t->data_bytes, slice, frames, 0};
    /* the first tile delivers the file header too; later ones only their blocks */
    const uint64_t skip = step.block0 ? AAD_HEADER_SIZE : 0;
    t->items[k] = {i, t->data_bytes + skip, step.block0 ? AAD_HEADER_SIZE + step.block0 * block_size : 0, slice - skip, !skip && slice < sizes[i]};
    t->drain_cost[k] = t->data_bytes;
    t->fill_cost[k] = t->pcm_elems * sizeof(int16_t);
    t->pcm_elems += round_up((uint64_t)frames * ch, 8);
    t->data_bytes += round_up(slice, 16);
  }
  t->drain_cost[n] = t->data_bytes;
  t->fill_cost[n] = t->pcm_elems * sizeof(int16_t);
  t->lone = step.group_first && step.group_last;
  t->carry = !t->lone;
  t->state_in = has_state && step.group_first;
  t->state_back = has_state && step.group_last;
  /* input block: table | state | pcm ; output block: image slices | state.  Every stream of a group is alive in its first tile,
   * so the incoming states are n == order.size() records */
  t->table_bytes = round_up(sizeof(AADHipStreamDesc) * (uint64_t)n, 64);
  t->payload_off = t->table_bytes + round_up(t->state_in ? sizeof(AADHipLaneState) * (uint64_t)n * ch : 0, 64);
  t->in_bytes = t->payload_off + t->pcm_elems * sizeof(int16_t);
  t->out_bytes = t->data_bytes + (t->state_back ? sizeof(AADHipLaneState) * (uint64_t)t->group_size * ch : 0);
  t->down_bytes = t->lone ? t->out_bytes : t->data_bytes; /* carried states come from the device records, by a copy of their own */
  if (t->state_back) t->state_order = order; else t->state_order.clear();
}

/* what the host still has to do with a decoded tile: int16 elements [src, src + frames * channels) of the output block are frames
 * [frame0, frame0 + frames) of stream `stream` */
struct FrameRun {
  uint32_t stream;
  uint64_t src, frame0, frames;
};

struct DecodeTile : TileLayout {
  static constexpr bool kCutUp = false; /* a lone tile's output copy is the one cut into pieces */
  std::vector<FrameRun> items;
  std::vector<uint64_t> tile_blocks; /* per row: blocks of its stream that the tile decodes */
  uint64_t fill_byte0;               /* every row holds its image's bytes [fill_byte0, fill_byte0 + table[k].data_size) */
};

/* Bytes a full block's decode touches beyond its own block_size (0 for every geometry an encoder writes), and in *block_cost
 * what one block of a stream takes of the tile budget: its PCM, its bytes, that reach. */
inline uint64_t decode_overreach(uint32_t ch, uint32_t bits, uint32_t spb, uint32_t block_size, uint64_t *block_cost)
{
  const uint64_t unit_samples = bits == 3 ? 8 : (bits == 4 ? 2 : 4);
  const uint64_t unit_bytes = (uint64_t)(bits == 3 ? 3 : 1) * ch;
  const uint64_t touched = (uint64_t)AAD_BLOCK_HEADER_BYTES_PER_CH * ch + (spb > 4 ? (spb - 4 + unit_samples - 1) / unit_samples * unit_bytes : 0);
  const uint64_t overreach = touched > block_size ? touched - block_size : 0;
  *block_cost = (uint64_t)spb * ch * sizeof(int16_t) + block_size + overreach;
  return overreach;
}

/* data_size / num_samples / blocks (what decode_plan_init counts: blocks present, the last maybe short, at most what the samples
 * need): per stream of the batch; head: AAD_HEADER_SIZE for file images, 0 for bare blocks.  Tiles carry bare blocks. */
inline void decode_tile_layout(const TileStep &step, const std::vector<uint32_t> &order, const uint64_t *data_size, const uint32_t *num_samples,
                               const uint64_t *blocks, uint32_t ch, uint32_t spb, uint32_t block_size, uint32_t head, uint64_t overreach, DecodeTile *t)
{
  const uint32_t n = step.alive;
  t->start(step);
  t->items.resize(n);
  t->tile_blocks.resize(n);
  t->fill_byte0 = head + step.block0 * block_size;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t i = order[k];
    const uint64_t payload = data_size[i] - head; /* alive: it has a block, so more than `head` bytes */
    /* a block whose header asks for more samples than block_size holds reads on into the bytes behind it, as the reference's
     * unbounded code walk does (src/aad_decoder.c:396-451; the header checks relate samples_per_block and block_size to
     * nothing, :173-225): a tile carries that reach behind its last block, and a stream's last tile every byte that is left */
    const uint64_t byte0 = step.block0 * block_size;
    const uint64_t upto = step.block1 >= blocks[i] ? payload : step.block1 * block_size + overreach;
    const uint64_t byte1 = upto < payload ? upto : payload;
    const uint64_t frame0 = step.block0 * spb, frame1 = step.block1 * spb < num_samples[i] ? step.block1 * spb : num_samples[i];
    /* frames the reference's block walk produces: it stops when the bytes run out (src/aad_decoder.c:514) */
    t->tile_blocks[k] = (step.block1 < blocks[i] ? step.block1 : blocks[i]) - step.block0;
    const uint64_t by_bytes = t->tile_blocks[k] * spb;
    t->table[k] = AADHipStreamDesc{t->pcm_elems, t->data_bytes, byte1 - byte0, (uint32_t)(frame1 - frame0), 0};
    t->items[k] = {i, t->pcm_elems, frame0, by_bytes < frame1 - frame0 ? by_bytes : frame1 - frame0};
    t->drain_cost[k] = t->pcm_elems * sizeof(int16_t);
    t->fill_cost[k] = t->data_bytes;
    t->pcm_elems += round_up((frame1 - frame0) * ch, 8);
    t->data_bytes += round_up(byte1 - byte0, 16);
  }
  t->drain_cost[n] = t->pcm_elems * sizeof(int16_t);
  t->fill_cost[n] = t->data_bytes;
  /* input block: table | block prefix (alive + 1 counts) | bare blocks ; output block: pcm */
  t->table_bytes = round_up(sizeof(AADHipStreamDesc) * (uint64_t)n, 64);
  t->payload_off = t->table_bytes + round_up(sizeof(uint64_t) * ((uint64_t)n + 1), 64);
  t->in_bytes = t->payload_off + t->data_bytes;
  t->out_bytes = t->down_bytes = t->pcm_elems * sizeof(int16_t);
}

/* The pieces of a tile's input copy (up) or of its output copy: only a batch that goes as one tile (not piped) cuts a copy, and
 * of its two the big one - the input's where Tile::kCutUp, else the output's.  The other copy is one piece. */
template <class Tile>
uint32_t copy_pieces(const Tile &t, bool up, bool piped, uint32_t *end)
{
  return cut_pieces(up ? t.fill_cost : t.drain_cost, t.step.alive, up == Tile::kCutUp && !piped, end);
}

} /* namespace aad */

#endif /* AAD_TILES_H */
