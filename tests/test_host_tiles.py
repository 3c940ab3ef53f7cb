"""Tile planning of the host-memory path on the CPU (aad_amd/csrc/aad_tiles.h): how AADHip_EncodeBatch / AADHip_DecodeBatch, the
legacy whole-file calls and aad_batch cut a batch into groups and tiles (TilePlanner), what each tile's two pinned blocks hold
(encode_tile_layout, decode_tile_layout, decode_overreach) and how a lone tile's big copy is cut into pieces (cut_pieces), through
tests/host_tiles_driver.cpp built with g++ against that header.  The driver walks a batch as the pipeline does (run_tiles in
aad_hip_engine.hip) and prints numbers; everything expected of them is written out here, from the format's arithmetic alone.

A decode stream's blocks are the blocks PRESENT in its image, a short last one included, and at most what its samples need - the
count decode_plan_init hands the planner (the reference walks blocks while samples AND bytes remain, src/aad_decoder.c:514) - so a
stream receives frames [0, min(num_samples, blocks present * spb))."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
HEAD = 31                      # AAD_HEADER_SIZE
BLOCK_HEAD = 18                # AAD_BLOCK_HEADER_BYTES_PER_CH
DESC, STATE = 32, 40           # sizeof(AADHipStreamDesc), sizeof(AADHipLaneState)
UNIT = {4: (1, 2), 3: (3, 8), 2: (1, 4)}   # bits -> (bytes per channel, samples) of one pack unit: lcm(8, bits) bits
CHUNK = 16 << 20               # kChunkBudget == kCutAbove
UNBOUNDED = ((1 << 64) - 1) >> 8
PIECE, MAX_PIECES = 1 << 20, 4


def up(v, a):
    return -(-v // a) * a


def geometry(max_block_size, ch, bits):
    """block_size and samples per block of AADFormat_BlockGeometry"""
    unit_bytes, unit_samples = UNIT[bits]
    units = (max_block_size - BLOCK_HEAD * ch) // (unit_bytes * ch)
    return BLOCK_HEAD * ch + units * unit_bytes * ch, 4 + units * unit_samples


def block_bytes(n, ch, bits):
    unit_bytes, unit_samples = UNIT[bits]
    return (BLOCK_HEAD + (-(-(n - 4) // unit_samples) if n > 4 else 0) * unit_bytes) * ch


def encoded_size(n, ch, bits, spb):
    return HEAD + (n // spb) * block_bytes(spb, ch, bits) + (block_bytes(n % spb, ch, bits) if n % spb else 0)


def geometries():
    """(ch, bits, block_size, spb): per channel count and bit depth the smallest block the format allows (one pack unit) and a large one"""
    out = []
    for ch, bits in itertools.product((1, 2, 8), (2, 3, 4)):
        smallest = BLOCK_HEAD * ch + UNIT[bits][0] * ch
        for max_block_size in (smallest, 4096):
            bs, spb = geometry(max_block_size, ch, bits)
            assert bs <= max_block_size and block_bytes(spb, ch, bits) == bs
            out.append((ch, bits, bs, spb))
    assert min(g[3] for g in out) == 6 and max(g[3] for g in out) > 16000
    return out


def batches(spb):
    """stream lengths in frames"""
    return [[],                                                             # empty
            [5 * spb + 3],                                                  # one stream
            [1], [spb - 1, 2, spb // 2 + 1],                                # shorter than a block
            [spb], [spb + 1],
            [3, 5 * spb + 7, spb, 1, 2 * spb, 12 * spb - 1, spb + 1],       # ragged
            [7 * spb, 2, 7 * spb, 3 * spb + 1, 3 * spb, 1, 9 * spb - 2],
            [2 * spb] * 40,                                                 # many equal streams
            [spb // 3 + 1] * 10 + [40 * spb + 5] + [spb // 3 + 1] * 10]     # one long stream among short ones


def budgets(cost):
    """tile_bytes: from less than one block of one stream to the built-in budget (0: unbounded for these batches)"""
    return [cost // 3, cost, 3 * cost + 5, 10 * cost, 64 << 10, 0]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_tiles") / "host_tiles_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o",
                    str(exe), os.path.join(ROOT, "tests", "host_tiles_driver.cpp")], check=True)
    return str(exe)


TILE_FIELDS = ("alive block0 block1 group_first group_last lead fill_from lone carry state_in state_back group_size pcm_elems data_bytes "
               "table_bytes payload_off in_bytes out_bytes down_bytes").split()
ROW_FIELDS = "stream pcm_offset data_offset data_size num_samples src dst count patch fill_cost drain_cost tile_blocks".split()


def run(driver, mode, lines):
    """one parsed record per input line: {"batch": [...], "tiles": [{..., "order", "states", "up", "down", "costs", "rows"}]}"""
    text = subprocess.run([driver, mode], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    cases, case = [], None
    for line in text.splitlines():
        key, *rest = line.split()
        v = [int(x) for x in rest]
        if key == "batch":
            case = {"batch": v, "tiles": []}
        elif key == "tile":
            case["tiles"].append(dict(zip(TILE_FIELDS, v), rows=[]))
        elif key == "row":
            case["tiles"][-1]["rows"].append(dict(zip(ROW_FIELDS, v)))
        elif key == "end":
            cases.append(case)
        else:
            case["tiles"][-1][key] = v
    assert len(cases) == len(lines)
    return cases


def expected_budget(tile_bytes, total):
    if tile_bytes > 0:
        return tile_bytes, True
    return (CHUNK, True) if total > CHUNK else (UNBOUNDED, False)


def expected_pieces(prefix, wanted):
    """the rule of cut_pieces: total // 1 MiB pieces, four at most, each ending at the first item that starts at or behind its share"""
    count, total = len(prefix) - 1, prefix[-1]
    pieces = min(max(total // PIECE if wanted else 1, 1), MAX_PIECES)
    ends = []
    for p in range(1, pieces):
        at = next((k for k in range(count) if prefix[k] >= total // pieces * p), count)
        if at > (ends[-1] if ends else 0) and at < count:
            ends.append(at)
    return ends + [count]


def check_pieces(ends, prefix, wanted):
    count = len(prefix) - 1
    assert 1 <= len(ends) <= MAX_PIECES and ends[-1] == count
    assert all(a < b for a, b in zip(ends, ends[1:])), "piece ends strictly increasing"
    if not wanted or prefix[-1] < 2 * PIECE:
        assert ends == [count], "one piece when not wanted or under the piece size"
    assert ends == expected_pieces(prefix, wanted)


def check_planner(case, blocks, cost, tile_bytes, total, has_state, encode):
    """the walk of one batch: groups of consecutive streams, longest first, tiles of block ranges within the budget"""
    budget, piped = expected_budget(tile_bytes, total)
    assert case["batch"][:2] == [budget, int(piped)]
    assert case["batch"][3] == cost
    next_stream, tiles, k = 0, case["tiles"], 0
    while k < len(tiles):
        t = tiles[k]
        assert t["group_first"] == 1, "a group opens with group_first"
        order = t["order"]
        # the group: consecutive streams until one block of each (empty ones cost nothing) reaches the budget ...
        size, acc = 0, 0
        while True:
            acc += cost if blocks[next_stream + size] else 0
            size += 1
            if next_stream + size >= len(blocks) or acc >= budget:
                break
        members = list(range(next_stream, next_stream + size))
        if not any(blocks[i] for i in members):   # ... a group of empty streams has no tile
            next_stream += size
            continue
        # ... longest first, equal lengths in batch order
        assert order == sorted(members, key=lambda i: -blocks[i]), "the group's order"
        next_stream += size
        longest, block0 = blocks[order[0]], 0
        while True:
            t = tiles[k]
            assert t["order"] == order
            assert t["group_first"] == int(block0 == 0) and t["block0"] == block0, "group_first brackets the group, tiles are contiguous"
            alive = sum(1 for i in order if blocks[i] > block0)
            assert t["alive"] == alive and [r["stream"] for r in t["rows"]] == order[:alive], "alive streams: a prefix of the order"
            span = t["block1"] - t["block0"]
            assert span >= 1 and t["block1"] <= longest
            if alive * cost > budget:
                assert span == 1, "one block of each alive stream exceeds the budget: one block per tile"
            else:
                assert alive * span * cost <= budget, "a tile's payload stays within the budget"
                assert t["block1"] == longest or alive * (span + 1) * cost > budget, "and takes all the blocks that fit"
            assert t["group_last"] == int(t["block1"] == longest), "group_last brackets the group"
            first, last = bool(t["group_first"]), bool(t["group_last"])
            if encode:
                assert t["lone"] == int(first and last) and t["carry"] == int(not (first and last))
                assert t["state_in"] == int(has_state and first) and t["state_back"] == int(has_state and last)
                assert t["group_size"] == len(order)
                assert t["states"] == (order if has_state and last else [])
            block0 = t["block1"]
            k += 1
            if last:
                break
    assert all(blocks[i] == 0 for i in range(next_stream, len(blocks))), "every stream with blocks was in a group"
    return piped


def check_layout(t, ch, piped, pcm_up):
    """what both directions share: aligned, disjoint rows, the cost prefixes, the piece cuts"""
    rows = t["rows"]
    pcm_end = data_end = 0
    for r in rows:
        assert r["pcm_offset"] % 8 == 0 and r["data_offset"] % 16 == 0
        assert r["pcm_offset"] >= pcm_end and r["data_offset"] >= data_end, "rows do not overlap"
        pcm_end, data_end = r["pcm_offset"] + r["num_samples"] * ch, r["data_offset"] + r["data_size"]
        pcm_cost, data_cost = (r["fill_cost"], r["drain_cost"]) if pcm_up else (r["drain_cost"], r["fill_cost"])
        assert pcm_cost == r["pcm_offset"] * 2 and data_cost == r["data_offset"]
    assert t["pcm_elems"] >= pcm_end and t["data_bytes"] >= data_end
    assert t["pcm_elems"] == sum(up(r["num_samples"] * ch, 8) for r in rows) and t["data_bytes"] == sum(up(r["data_size"], 16) for r in rows)
    fill = [r["fill_cost"] for r in rows] + [t["costs"][0]]
    drain = [r["drain_cost"] for r in rows] + [t["costs"][1]]
    for prefix in (fill, drain):
        assert prefix[0] == 0 and all(a <= b for a, b in zip(prefix, prefix[1:])), "cost prefixes are non-decreasing"
    assert (fill[-1], drain[-1]) == ((t["pcm_elems"] * 2, t["data_bytes"]) if pcm_up else (t["data_bytes"], t["pcm_elems"] * 2)), \
        "and end at the payload size"
    check_pieces(t["up"], fill, pcm_up and not piped)
    check_pieces(t["down"], drain, not pcm_up and not piped)


def encode_cases():
    for (ch, bits, bs, spb), trials, has_state in itertools.product(geometries(), (0, 1), (0, 1)):
        cost = spb * ch * 2 + bs
        for ns, tile_bytes in itertools.product(batches(spb), budgets(cost)):
            yield ch, bits, bs, spb, trials, has_state, tile_bytes, ns
    # past the built-in cut (16 MiB): a wide batch of one-block stereo streams, and a few long streams
    bs, spb = geometry(1024, 2, 4)
    for ns in ([spb] * 5000, [700 * spb + 11, 900 * spb, 650 * spb + 1]):
        yield 2, 4, bs, spb, 1, 1, 0, ns
    # one tile of several MiB: its input copy goes up in pieces
    for ns in ([spb] * 900, [spb * 3] * 1000, [spb * 400, 5, spb * 300], [spb * 1500]):
        yield 2, 4, bs, spb, 0, 0, 0, ns


def test_encode_tiles_cover_every_image_once(driver):
    cases = list(encode_cases())
    lines = []
    for ch, bits, bs, spb, trials, has_state, tile_bytes, ns in cases:
        sizes = [encoded_size(n, ch, bits, spb) for n in ns]
        total = sum(n * ch * 2 + s for n, s in zip(ns, sizes))
        lines.append("%d %d %d %d %d %d %d %d %d %s" % (ch, spb, bs, spb * ch * 2 + bs, tile_bytes, total, trials, has_state, len(ns),
                                                        " ".join("%d %d %d" % (n, s, -(-n // spb)) for n, s in zip(ns, sizes))))
    seen = {"cut": 0, "whole": 0, "lead": 0, "patch": 0, "up pieces": 0, "one block per tile": 0}
    for (ch, bits, bs, spb, trials, has_state, tile_bytes, ns), case in zip(cases, run(driver, "encode", lines)):
        sizes = [encoded_size(n, ch, bits, spb) for n in ns]
        blocks = [-(-n // spb) for n in ns]
        cost = spb * ch * 2 + bs
        piped = check_planner(case, blocks, cost, tile_bytes, sum(n * ch * 2 + s for n, s in zip(ns, sizes)), has_state, True)
        seen["cut" if piped else "whole"] += 1
        delivered = [0] * len(ns)    # image bytes of each stream handed over so far
        for t in case["tiles"]:
            check_layout(t, ch, piped, True)
            n, block0, block1 = t["alive"], t["block0"], t["block1"]
            lead = spb if trials and block0 > 0 else 0
            assert t["lead"] == lead and t["fill_from"] == block0 * spb - lead, "the fill range starts one block back for the trial search"
            seen["lead"] += lead > 0
            seen["up pieces"] += len(t["up"]) > 1
            seen["one block per tile"] += n * cost > case["batch"][0]
            assert t["down"] == [n], "an encoded tile comes down in one piece"
            for r in t["rows"]:
                i = r["stream"]
                frames = min(block1 * spb, ns[i]) - block0 * spb
                assert frames > 0 and r["num_samples"] == frames + lead
                # the slice: a file header and the tile's blocks, the stream's short last block as it is
                body = sum(block_bytes(min(spb, ns[i] - b * spb), ch, bits) for b in range(block0, min(block1, blocks[i])))
                assert r["data_size"] == HEAD + body
                # the file header is delivered with the first tile only; in order, nothing twice, nothing left out
                skip = HEAD if block0 else 0
                assert r["src"] == r["data_offset"] + skip and r["count"] == r["data_size"] - skip
                assert r["dst"] == delivered[i] == (HEAD + block0 * bs if block0 else 0)
                delivered[i] += r["count"]
                # the header of a first slice holds the tile's count: patched exactly when the stream goes on
                assert r["patch"] == int(block0 == 0 and r["count"] < sizes[i])
                seen["patch"] += r["patch"]
            state_in = STATE * n * ch if t["state_in"] else 0
            state_back = STATE * t["group_size"] * ch if t["state_back"] else 0
            assert t["table_bytes"] == up(DESC * n, 64)
            assert t["payload_off"] == t["table_bytes"] + up(state_in, 64)
            assert t["in_bytes"] == t["payload_off"] + t["pcm_elems"] * 2
            assert t["out_bytes"] == t["data_bytes"] + state_back
            assert t["down_bytes"] == (t["out_bytes"] if t["lone"] else t["data_bytes"])
            if t["state_in"]:
                assert n == t["group_size"], "every stream of a group is alive in its first tile"
        assert delivered == sizes, "every image is covered exactly once"
    assert all(seen.values()), seen


def decode_cases():
    """(ch, bits, bs, spb, head, tile_bytes, [(num_samples, data_size)])"""
    for (ch, bits, bs, spb), head in itertools.product(geometries(), (0, HEAD)):
        variants = [(bs, spb, 0)]
        # a header that claims more samples per block than block_size holds: the decode reads on behind the block
        variants.append((bs, spb + 40 * UNIT[bits][1], 7))
        for (vbs, vspb, extra) in variants:
            cost = vspb * ch * 2 + vbs + max(0, block_bytes(vspb, ch, bits) - vbs)
            for ns in batches(vspb):
                whole = [head + -(-n // vspb) * vbs + extra for n in ns]            # every block at full size, `extra` bytes behind
                exact = [head + (encoded_size(n, ch, bits, vspb) - HEAD if vspb == spb else -(-n // vspb) * vbs) for n in ns]
                # truncated: fewer blocks than the samples need, cut at a block boundary or inside a block behind its header
                short = [head + (-(-n // vspb) // 2) * vbs + (BLOCK_HEAD * ch + 1 if k % 2 and n > vspb else 0) for k, n in enumerate(ns)]
                for sizes in (whole, exact, short):
                    for tile_bytes in budgets(cost):
                        yield ch, bits, vbs, vspb, head, tile_bytes, list(zip(ns, sizes))
    bs, spb = geometry(1024, 2, 4)
    for streams in ([(spb, HEAD + bs)] * 5000, [(700 * spb + 11, HEAD + 701 * bs), (900 * spb, HEAD + 450 * bs)]):
        yield 2, 4, bs, spb, HEAD, 0, streams          # past the built-in cut
    for streams in ([(spb, HEAD + bs)] * 900, [(spb * 3, HEAD + bs * 3)] * 1000, [(spb * 1500, HEAD + bs * 1500)]):
        yield 2, 4, bs, spb, HEAD, 0, streams          # one tile of several MiB: its output copy comes down in pieces


def test_decode_tiles_deliver_every_frame_once(driver):
    cases = list(decode_cases())
    lines, all_blocks = [], []
    for ch, bits, bs, spb, head, tile_bytes, streams in cases:
        # blocks: while samples remain and bytes remain
        blocks = [min(-(-n // spb), -(-(size - head) // bs)) for n, size in streams]
        all_blocks.append(blocks)
        total = sum(size + n * ch * 2 for n, size in streams)
        lines.append("%d %d %d %d %d %d %d %d %s" % (ch, bits, spb, bs, head, tile_bytes, total, len(streams),
                                                     " ".join("%d %d %d" % (n, size, b) for (n, size), b in zip(streams, blocks))))
    seen = {"cut": 0, "whole": 0, "overreach": 0, "clipped": 0, "truncated": 0, "short last block": 0, "down pieces": 0, "no blocks": 0}
    for (ch, bits, bs, spb, head, tile_bytes, streams), blocks, case in zip(cases, all_blocks, run(driver, "decode", lines)):
        overreach = max(0, block_bytes(spb, ch, bits) - bs)          # what a full block's decode touches beyond block_size
        cost = spb * ch * 2 + bs + overreach
        assert case["batch"][2] == overreach
        seen["overreach"] += overreach > 0
        piped = check_planner(case, blocks, cost, tile_bytes, sum(size + n * ch * 2 for n, size in streams), 0, False)
        seen["cut" if piped else "whole"] += 1
        frames_got = [0] * len(streams)
        bytes_sent = [0] * len(streams)
        for t in case["tiles"]:
            check_layout(t, ch, piped, False)
            n, block0, block1 = t["alive"], t["block0"], t["block1"]
            assert t["fill_from"] == head + block0 * bs and t["lead"] == 0
            assert t["up"] == [n], "a tile of images goes up in one piece"
            seen["down pieces"] += len(t["down"]) > 1
            for r in t["rows"]:
                i = r["stream"]
                num_samples, payload = streams[i][0], streams[i][1] - head
                # its blocks and the reach behind the last, clipped to the payload; a stream's last tile: every byte that is left
                want = payload - block0 * bs if block1 >= blocks[i] else min((block1 - block0) * bs + overreach, payload - block0 * bs)
                assert r["data_size"] == want
                seen["clipped"] += block1 < blocks[i] and overreach > 0 and want < (block1 - block0) * bs + overreach
                assert r["tile_blocks"] == min(block1, blocks[i]) - block0
                assert r["num_samples"] == min(block1 * spb, num_samples) - block0 * spb
                assert r["src"] == r["pcm_offset"] and r["dst"] == block0 * spb
                assert r["count"] == min(r["num_samples"], r["tile_blocks"] * spb)
                assert r["dst"] == frames_got[i], "frames in order, none twice"
                frames_got[i] += r["count"]
                bytes_sent[i] = block0 * bs + r["data_size"]
            assert t["table_bytes"] == up(DESC * n, 64)
            assert t["payload_off"] == t["table_bytes"] + up(8 * (n + 1), 64)
            assert t["in_bytes"] == t["payload_off"] + t["data_bytes"]
            assert t["out_bytes"] == t["down_bytes"] == t["pcm_elems"] * 2
        for i, (num_samples, size) in enumerate(streams):
            present = -(-(size - head) // bs)
            assert frames_got[i] == min(num_samples, present * spb), "every stream receives its frames exactly once"
            if blocks[i]:
                assert bytes_sent[i] == size - head, "a stream's last tile carries every byte that is left"
            seen["truncated"] += present * spb < num_samples
            seen["short last block"] += blocks[i] > 0 and (size - head) % bs != 0 and present * spb < num_samples
            seen["no blocks"] += blocks[i] == 0
    assert all(seen.values()), seen


def test_cut_pieces(driver):
    MiB = 1 << 20
    prefixes = [[0, 10], [0, MiB - 1], [0, MiB], [0, 2 * MiB - 1], [0, 2 * MiB], [0, 100 * MiB],          # one item: one piece
                [0, MiB, 2 * MiB], [0, MiB, 2 * MiB, 3 * MiB, 4 * MiB, 5 * MiB],
                list(range(0, 9 * MiB, MiB // 3)),                                                        # many small items
                [0, 8 * MiB, 8 * MiB + 1, 8 * MiB + 2],                                                   # one item holds nearly all
                [0, 1, 2, 8 * MiB],
                [0, 0, 0, 3 * MiB, 3 * MiB, 6 * MiB],                                                     # items of no cost
                [0, 3 * MiB // 2, 3 * MiB], [0, 5 * MiB // 2, 5 * MiB // 2 + 7]]
    cases = [(wanted, p) for p in prefixes for wanted in (0, 1)]
    lines = ["%d %d %s" % (wanted, len(p) - 1, " ".join(str(v) for v in p)) for wanted, p in cases]
    out = subprocess.run([driver, "pieces"], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (wanted, prefix), line in zip(cases, out):
        check_pieces([int(v) for v in line.split()[1:]], prefix, bool(wanted))
    assert any(len(line.split()) - 1 == MAX_PIECES for line in out)
