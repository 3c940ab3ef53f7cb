/* Host driver of the tile planning's CPU tests (tests/test_host_tiles.py), built with g++ against the header the host-memory
 * pipeline itself plans with (aad_amd/csrc/aad_tiles.h).  It walks a batch exactly as run_tiles does - planner, one layout per
 * tile, the piece cuts of the two copies - and prints what it finds as plain numbers.
 *   encode -> for each line "<ch> <spb> <block_size> <block_cost> <tile_bytes> <total> <trials> <has_state> <n>" followed by n
 *             triples "<num_samples> <image_size> <blocks>" on stdin
 *   decode -> for each line "<ch> <bits> <spb> <block_size> <head> <tile_bytes> <total> <n>" followed by n triples
 *             "<num_samples> <data_size> <blocks>"
 *             both print "batch <budget> <piped> <overreach> <block_cost>", then per tile
 *               "tile <alive> <block0> <block1> <group_first> <group_last> <lead> <fill_from> <lone> <carry> <state_in> <state_back>
 *                     <group_size> <pcm_elems> <data_bytes> <table_bytes> <payload_off> <in_bytes> <out_bytes> <down_bytes>"
 *               "order <the planner's group>", "states <state_order>", "up <piece ends>", "down <piece ends>",
 *               "costs <fill_cost[alive]> <drain_cost[alive]>" and per row
 *               "row <stream> <pcm_offset> <data_offset> <data_size> <num_samples> <src> <dst> <count> <patch_count> <fill_cost>
 *                    <drain_cost> <tile_blocks>"
 *             and "end" behind the last tile
 *   pieces -> for each line "<wanted> <count> <prefix[0]> ... <prefix[count]>": the piece ends of cut_pieces on one line */
#include <cstdio>
#include <cstring>
#include <vector>

#include "aad_tiles.h"

typedef unsigned long long ull;

struct Batch {
  std::vector<uint32_t> num_samples;
  std::vector<uint64_t> sizes, blocks;
};

static bool read_batch(unsigned n, Batch *b)
{
  b->num_samples.resize(n);
  b->sizes.resize(n);
  b->blocks.resize(n);
  for (unsigned i = 0; i < n; i++) {
    unsigned samples;
    ull size, blocks;
    if (scanf("%u %llu %llu", &samples, &size, &blocks) != 3) return false;
    b->num_samples[i] = samples;
    b->sizes[i] = size;
    b->blocks[i] = blocks;
  }
  return true;
}

static void print_list(const char *name, const uint32_t *v, size_t n)
{
  printf("%s", name);
  for (size_t i = 0; i < n; i++) printf(" %u", v[i]);
  printf("\n");
}

/* the parts of a tile that both directions have, and the piece cuts of its two copies as run_tiles asks for them */
template <class Tile>
static void print_tile(const Tile &t, const std::vector<uint32_t> &order, bool piped, ull lead, ull fill_from, const bool flags[4], ull group_size,
                       const std::vector<uint32_t> &state_order)
{
  const aad::TileStep &s = t.step;
  printf("tile %u %llu %llu %d %d %llu %llu %d %d %d %d %llu %llu %llu %llu %llu %llu %llu %llu\n", s.alive, (ull)s.block0, (ull)s.block1,
         (int)s.group_first, (int)s.group_last, lead, fill_from, (int)flags[0], (int)flags[1], (int)flags[2], (int)flags[3], group_size,
         (ull)t.pcm_elems, (ull)t.data_bytes, (ull)t.table_bytes, (ull)t.payload_off, (ull)t.in_bytes, (ull)t.out_bytes, (ull)t.down_bytes);
  print_list("order", order.data(), order.size());
  print_list("states", state_order.data(), state_order.size());
  uint32_t end[aad::kMaxPieces];
  print_list("up", end, aad::copy_pieces(t, true, piped, end));
  print_list("down", end, aad::copy_pieces(t, false, piped, end));
  printf("costs %llu %llu\n", (ull)t.fill_cost[s.alive], (ull)t.drain_cost[s.alive]);
}

static void print_row(const AADHipStreamDesc &d, uint32_t stream, ull src, ull dst, ull count, int patch, ull fill, ull drain, ull blocks)
{
  printf("row %u %llu %llu %llu %u %llu %llu %llu %d %llu %llu %llu\n", stream, (ull)d.pcm_offset, (ull)d.data_offset, (ull)d.data_size,
         d.num_samples, src, dst, count, patch, fill, drain, blocks);
}

static int encode()
{
  unsigned ch, spb, bs, trials, has_state, n;
  ull cost, total;
  long long tile_bytes;
  while (scanf("%u %u %u %llu %lld %llu %u %u %u", &ch, &spb, &bs, &cost, &tile_bytes, &total, &trials, &has_state, &n) == 9) {
    Batch b;
    if (!read_batch(n, &b)) return 1;
    const bool piped = aad::batch_is_cut(tile_bytes, total);
    aad::TilePlanner planner(b.blocks.data(), n, cost, aad::tile_budget(tile_bytes, total));
    printf("batch %llu %d 0 %llu\n", (ull)planner.budget, (int)piped, cost);
    aad::TileStep step;
    aad::EncodeTile t;
    while (planner.next(&step)) {
      aad::encode_tile_layout(step, planner.order, b.num_samples.data(), b.sizes.data(), b.blocks.data(), ch, spb, bs, trials != 0,
                              has_state != 0, &t);
      const bool flags[4] = {t.lone, t.carry, t.state_in, t.state_back};
      print_tile(t, planner.order, piped, t.lead, t.fill_frame0, flags, t.group_size, t.state_order);
      for (uint32_t k = 0; k < step.alive; k++) {
        const aad::ImageSlice &d = t.items[k];
        print_row(t.table[k], d.stream, d.src, d.dst, d.bytes, (int)d.patch_count, t.fill_cost[k], t.drain_cost[k], 0);
      }
    }
    printf("end\n");
  }
  return 0;
}

static int decode()
{
  unsigned ch, bits, spb, bs, head, n;
  ull total;
  long long tile_bytes;
  while (scanf("%u %u %u %u %u %lld %llu %u", &ch, &bits, &spb, &bs, &head, &tile_bytes, &total, &n) == 8) {
    Batch b;
    if (!read_batch(n, &b)) return 1;
    uint64_t cost;
    const uint64_t overreach = aad::decode_overreach(ch, bits, spb, bs, &cost);
    const bool piped = aad::batch_is_cut(tile_bytes, total);
    aad::TilePlanner planner(b.blocks.data(), n, cost, aad::tile_budget(tile_bytes, total));
    printf("batch %llu %d %llu %llu\n", (ull)planner.budget, (int)piped, (ull)overreach, (ull)cost);
    aad::TileStep step;
    aad::DecodeTile t;
    while (planner.next(&step)) {
      aad::decode_tile_layout(step, planner.order, b.sizes.data(), b.num_samples.data(), b.blocks.data(), ch, spb, bs, head, overreach, &t);
      const bool flags[4] = {false, false, false, false};
      print_tile(t, planner.order, piped, 0, t.fill_byte0, flags, 0, std::vector<uint32_t>());
      for (uint32_t k = 0; k < step.alive; k++) {
        const aad::FrameRun &d = t.items[k];
        print_row(t.table[k], d.stream, d.src, d.frame0, d.frames, 0, t.fill_cost[k], t.drain_cost[k], t.tile_blocks[k]);
      }
    }
    printf("end\n");
  }
  return 0;
}

static int pieces()
{
  unsigned wanted, count;
  while (scanf("%u %u", &wanted, &count) == 2) {
    std::vector<uint64_t> prefix((size_t)count + 1);
    for (unsigned i = 0; i <= count; i++) {
      ull v;
      if (scanf("%llu", &v) != 1) return 1;
      prefix[i] = v;
    }
    uint32_t end[aad::kMaxPieces];
    print_list("pieces", end, aad::cut_pieces(prefix, count, wanted != 0, end));
  }
  return 0;
}

int main(int argc, char **argv)
{
  if (argc == 2 && !strcmp(argv[1], "encode")) return encode();
  if (argc == 2 && !strcmp(argv[1], "decode")) return decode();
  if (argc == 2 && !strcmp(argv[1], "pieces")) return pieces();
  fprintf(stderr, "usage: encode | decode | pieces\n");
  return 2;
}
