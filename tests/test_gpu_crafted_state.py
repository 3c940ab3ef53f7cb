"""GPU parity on the crafted-state corpus (tests/crafted_state.py): every caller that hands a table of carried predictor state to the
encoders, started from records that music and noise never leave behind - first block headers at weight shifts 0 .. 15, both sides
of the shift 0 / 1 boundary, the step index and quantize_error at their ends, different records on the channels of one stream,
second calls of 1 .. 5 samples and next to a block boundary, step indices outside [0, 4080], weights past 2^30.

Bar: bit-exact, no tolerances.  The expected images are the oracle's (crafted_state.oracle_run), which the `corpus` fixture first
holds to the compiled reference's hashes and COMPLETE output records in tests/golden/crafted_state.json (the reference does not
exist here); output records are compared with the golden ones directly, every field.

One launch per format: all cases of a (channels, bits, M/S, trials, block size) group go into one launch in a permuted order, each
stream with its own records, the state table inside a larger tensor with canary records in front of and behind it, the images in
pattern-filled buffers (where the caller lets the test own them).  The plan of every device-resident launch is asked from
aad_launch_policy.h first (tests/launch_policy_driver.cpp) and must be the kernel the case claims; test_zz_what_ran prints, per
caller, mapping and trial lanes, the kernels named and the number of cases compared.  The host path's batches are cut by the
library itself: no plan is claimed for encode_host.

Where a block header cannot hold the weights.  A weight magnitude of 2^30 or more at a block start needs a header weight shift
of 16 and the 4-bit field holds shift & 15 (the reference asserts shift <= 15 and, built with NDEBUG, writes the wrapped field -
the golden images); INT32_MIN on a tap stays out of the largest magnitude, so the shift stays small and the tap's 16-bit field
reads 0.  Either way a decoder runs that block on other weights than the encoder holds, and the decode of the image is not the
encoder's own reconstruction.  The corpus holds both ways (crafted_state.oracle_reconstruction != the decode: test_crafted_state.py
names the streams).  It found the reconstruct kernels writing the encoder's reconstruction for such blocks: four of five groups
with a wrapped shift missed the bar under every mapping (249, 227, 624 and 62 row samples differing from the decode; in the 2ch
3-bit L/R trials 1 group channel 1's (sum_sq, sum_abs, max_abs) (23732324723, 1677589, 34866) against (101051612856, 3338440,
61145)).  The kernels now decide from what a decoder reads back from the header they wrote and walk such a block with the
decoder's recurrence as well (aad_encode.hip.h header_holds_weights, rec_wrapped_block).  test_state_callers holds the rows and
statistics of EVERY stream to the oracle's decode of the golden image; test_reconstruct_where_a_header_cannot_hold_the_weights
runs the groups with such a stream once more by name and says which streams they are.

The `beyond` tier cannot fault: the kernels form no address from a loaded record except through the step index, which the load
clamps (aad_encode.hip.h, encode_streams_kernel) and every table lookup masks into its table once more (aad_device.hip.h
wide_addr / wide4_addr / slot_addr; the index-delta lookups take the quantiser's magnitude, min(..., kMagMax)).  Weights, history
and quantize_error only enter arithmetic; the global addresses come from the stream table, the thread index and the sample
position.  The host path copies the records (state_in, d_state, state_back) and reads none of their fields."""
import collections

import numpy as np
import pytest

import aad_amd
import crafted_pcm as cp
import crafted_state as cs
import oracle_binding as ob
from aad_amd.capi import LANE_MAPPINGS, LANE_STATE_DTYPE, STREAM_DESC_DTYPE, TRIAL_LANES, make_parameter
from helpers import sha256
from test_oracle_golden import extract_channel_as_mono

pytestmark = pytest.mark.gpu

CALLERS = ["encode_uniform", "encode_plan", "encode_planar_i16", "encode_planar_f32", "reconstruct_planar", "codec_error", "encode_host"]
MAPPINGS = ["auto", "dense", "quad", "quad-fused"]
# the planar reconstruct plans always take single trial lanes (plan_reconstruct_encode): one pass over them is all there is
RUNS = [(c, m, l) for c in CALLERS for m in MAPPINGS for l in ("dual", "single") if not (l == "single" and c in ("reconstruct_planar", "codec_error"))]
GUARD = 3                 # canary records in front of and behind a state table
CANARY = 0x5AA5C33C       # every int32 of a canary record
IMG_FILL = 0xA5
LDS_PER_CU = 163840       # gfx950

Item = collections.namedtuple("Item", "case pcm image decoded records_in records_out apart")
TALLY = collections.Counter()  # (caller, mapping, trial lanes, kernel) -> cases compared


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def ring_engine(monkeypatch):
    """AAD_HIP_ENCODE_RING=2 (every geometry that can take the byte ring); a context reads it when it is created"""
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    monkeypatch.setenv("AAD_HIP_ENCODE_RING", "2")
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus():
    """{name: Item}: the oracle's image, decode and records per case, computed once and held to the compiled reference's"""
    golden = cs.golden()["cases"]
    out = {}
    for c in cs.cases():
        rec = golden[c["name"]]
        pcm = cs.case_pcm(c)
        assert sha256(pcm.tobytes()) == rec["pcm_sha256"], c["name"]
        image, lanes = cs.oracle_run(c, pcm=pcm)
        decoded = ob.decode(image)[0]
        apart = not np.array_equal(cs.oracle_reconstruction(c, pcm=pcm), decoded)  # a header that cannot hold the weights
        if c["channels"] <= 2:
            assert sha256(image) == rec["image_sha256"] and sha256(decoded.tobytes()) == rec["decoded_sha256"], c["name"]
        else:
            for ch in range(c["channels"]):
                assert sha256(extract_channel_as_mono(image, ch, rec["mono_block_size"])) == rec["mono_image_sha256"][ch], c["name"]
                assert sha256(np.ascontiguousarray(decoded[:, ch]).tobytes()) == rec["mono_decoded_sha256"][ch], c["name"]
        assert lanes == rec["records_out"], c["name"]
        out[c["name"]] = Item(c, pcm, image, decoded, rec["records_in"], rec["records_out"], apart)
    return out


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    """asks aad_launch_policy.h, the header the launches are planned with, for the plan of a batch on this device"""
    import os
    import subprocess
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path_factory.mktemp("crafted_state_policy") / "launch_policy_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(os.path.dirname(here), "aad_amd", "csrc"), "-o", exe,
                    os.path.join(here, "launch_policy_driver.cpp")], check=True)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    memo = {}

    def kernel(mapping, lanes, ring, rec, bits, ch, streams, trials, block_size):
        key = (mapping, lanes, ring, rec, bits, ch, streams, trials, block_size)
        if key not in memo:
            line = "%s %d %d %d %d %d -1 -1 0 %d %d %d %d %d 1\n" % ("R" if rec else "E", cus, LDS_PER_CU, LANE_MAPPINGS[mapping],
                                                                    TRIAL_LANES[lanes], ring, bits, ch, streams, trials, block_size)
            memo[key] = subprocess.run([exe], input=line, check=True, capture_output=True, text=True).stdout.split()[0]
        return memo[key]
    return kernel


def claimed(mapping, lanes, ring, rec, ch, trials):
    """the kernel a case of this module says it ran (these batches are far below the size at which "auto" turns dense)"""
    if ch > 2 or mapping == "dense":
        return "dense-ring" if ring == 2 and not rec and not trials and ch <= 2 else "dense"
    return "quad-dual" if trials and lanes == "dual" and not rec else "quad"


def groups(tiers=None):
    """{(channels, bits, ms, trials, max_block_size): [case]} in table order"""
    out = {}
    for c in cs.cases():
        if tiers is None or c["tier"] in tiers:
            out.setdefault((c["channels"], c["bits"], c["ms"], c["trials"], c["max_block_size"]), []).append(c)
    return out


def permuted(members, corpus, seed):
    order = np.random.default_rng(seed).permutation(len(members))
    return [corpus[members[int(i)]["name"]] for i in order]


def input_records(items, first=0):
    """LANE_STATE_DTYPE [streams * channels] of the items' input records: the index as the case has it (not clamped), garbage history"""
    ch = items[0].case["channels"]
    a = np.zeros(len(items) * ch, dtype=LANE_STATE_DTYPE)
    for i, it in enumerate(items):
        for c, r in enumerate(it.records_in):
            a[i * ch + c] = (r["w"], cs.garbage_history(first + i, c), r["idx"], r["qerr"])
    return a


def guarded(records):
    """int32 [GUARD + n + GUARD, 10] with the records in the middle and canary records around them"""
    host = np.full((2 * GUARD + len(records), 10), CANARY, dtype=np.int32)
    host[GUARD:GUARD + len(records)] = records.view(np.int32).reshape(-1, 10)
    return host


def unguarded(label, host, n):
    assert (host[:GUARD] == CANARY).all() and (host[GUARD + n:] == CANARY).all(), (label, "a canary record around the state table was written")
    return np.ascontiguousarray(host[GUARD:GUARD + n]).view(LANE_STATE_DTYPE).reshape(-1)


def check_records(label, records, items):
    ch = items[0].case["channels"]
    for i, it in enumerate(items):
        for c, want in enumerate(it.records_out):
            r = records[i * ch + c]
            got = {"w": [int(v) for v in r["weight"]], "h": [int(v) for v in r["history"]], "idx": int(r["stepsize_index"]),
                   "qerr": int(r["quantize_error"])}
            assert got == want, (label, it.case["name"], "stream %d channel %d" % (i, c), got, want, "in", it.records_in[c])


def check_images(label, images, items):
    for i, (img, it) in enumerate(zip(images, items)):
        assert bytes(img) == it.image, cp.describe_mismatch("%s, %s (stream %d)" % (label, it.case["name"], i), bytes(img), it.image)


def exact_stats(items):
    """int64 [N, C, 4] (sum_sq, sum_abs, max_abs, count) of x - decoded in python integers' range (|e| < 2^16, a few thousand samples)"""
    out = np.zeros((len(items), items[0].case["channels"], 4), dtype=np.int64)
    for i, it in enumerate(items):
        e = it.pcm.astype(np.int64).T - it.decoded.astype(np.int64).T
        out[i, :, 0], out[i, :, 1], out[i, :, 2], out[i, :, 3] = (e * e).sum(axis=1), np.abs(e).sum(axis=1), np.abs(e).max(axis=1), e.shape[1]
    return out


def check_rows(label, y, items, which):
    """rows of the streams `which` selects == the oracle's decode of the golden image, zero past each stream's end"""
    want = np.zeros(y.shape, dtype=np.int16)
    for i, it in enumerate(items):
        want[i, :, :it.decoded.shape[0]] = it.decoded.T
    pick = [i for i, it in enumerate(items) if which(it)]
    bad = np.argwhere(y[pick] != want[pick])
    assert y.dtype == np.int16 and bad.size == 0, (label, "rows differ from the decode of the image, first at [stream, channel, frame]",
                                                   [pick[bad[0][0]]] + bad[0][1:].tolist(), "samples that differ", len(bad),
                                                   "in streams", sorted({items[pick[b[0]]].case["name"] for b in bad}))


def planar_x(torch, items, f32):
    """[N, C, T] cuda rows, garbage past every stream's end; float32: x / 32768 (exact) as a view of a bigger tensor whose channel and
    stream strides exceed T and C T"""
    n, ch, t = len(items), items[0].case["channels"], max(it.pcm.shape[0] for it in items)
    if f32:
        host = np.full((n + 2, ch, t + 7), 9.25, dtype=np.float32)
        for i, it in enumerate(items):
            host[1 + i, :, 3:3 + it.pcm.shape[0]] = it.pcm.T.astype(np.float32) / np.float32(32768.0)
        x = torch.from_numpy(host).cuda()[1:n + 1, :, 3:3 + t]
        assert x.stride(-1) == 1 and x.stride(1) > t
        return x
    host = np.full((n, ch, t), 12345, dtype=np.int16)
    for i, it in enumerate(items):
        host[i, :, :it.pcm.shape[0]] = it.pcm.T
    return torch.from_numpy(host).cuda()


def round64(v):
    return -(-int(v) // 64) * 64


# ---- the seven callers: each takes the items of one launch -> (images or None, records after the call, rows or None, stats or None) --

def call_encode_plan(engine, torch, label, items, param, ring=False):
    """a ragged device-resident plan: odd PCM offsets, images on 64-byte boundaries with a sector of pattern between them; data_size
    is the image's size (with the byte ring: rounded up to the sector, whose tail the encoder may fill as it likes)"""
    ch, n = param.num_channels, len(items)
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    pos_p, pos_d, parts = 3, 64, [np.full(3, 77, dtype=np.int16)]
    for i, it in enumerate(items):
        size = engine.encoded_size(param, it.pcm.shape[0])
        assert size == len(it.image)
        d["pcm_offset"][i], d["data_offset"][i], d["num_samples"][i] = pos_p, pos_d, it.pcm.shape[0]
        d["data_size"][i] = round64(size) if ring else size
        parts += [it.pcm.reshape(-1), np.full(1 + i % 3, 77, dtype=np.int16)]
        pos_p += it.pcm.size + 1 + i % 3
        pos_d += round64(size) + 64
    d_pcm = torch.from_numpy(np.concatenate(parts)).cuda()
    d_img = torch.full((pos_d,), IMG_FILL, dtype=torch.uint8, device="cuda")
    big = torch.from_numpy(guarded(input_records(items))).cuda()
    plan = engine.encode_plan(param, d)
    try:
        plan.run(d_pcm, d_img, big[GUARD:GUARD + n * ch])
        torch.cuda.synchronize()
    finally:
        plan.close()
    img = d_img.cpu().numpy()
    outside = np.ones(img.size, dtype=bool)
    images = []
    for i in range(n):
        o = int(d["data_offset"][i])
        images.append(img[o:o + len(items[i].image)].tobytes())
        outside[o:o + int(d["data_size"][i])] = False
    assert (img[outside] == IMG_FILL).all(), (label, "a byte outside the images was written, first at", int(np.nonzero(outside & (img != IMG_FILL))[0][0]))
    return images, unguarded(label, big.cpu().numpy(), n * ch), None, None


def call_encode_uniform(engine, torch, label, items, param):
    """encode_uniform takes equal lengths: one launch per subset of equal-length streams, each with its own guarded table"""
    ch = param.num_channels
    images, records = [None] * len(items), np.zeros(len(items) * ch, dtype=LANE_STATE_DTYPE)
    by_length = {}
    for i, it in enumerate(items):
        by_length.setdefault(it.pcm.shape[0], []).append(i)
    for n, members in sorted(by_length.items()):
        sub = [items[i] for i in members]
        big = torch.from_numpy(guarded(input_records(sub, first=members[0]))).cuda()
        d_img, size = engine.encode_uniform(torch.from_numpy(np.stack([it.pcm for it in sub])).cuda(), param,
                                            state=big[GUARD:GUARD + len(sub) * ch])
        torch.cuda.synchronize()
        host = d_img.cpu().numpy()
        got = unguarded(label, big.cpu().numpy(), len(sub) * ch)
        for k, i in enumerate(members):
            images[i] = host[k, :size].tobytes()
            records[i * ch:(i + 1) * ch] = got[k * ch:(k + 1) * ch]
    return images, records, None, None


def call_encode_planar(engine, torch, label, items, param, f32, ring=False):
    """a planar encode plan over the test's own image buffer: rows of pattern in front of and behind the images' rows"""
    ch, n = param.num_channels, len(items)
    x = planar_x(torch, items, f32)
    sizes = [engine.encoded_size(param, it.pcm.shape[0]) for it in items]
    stride = round64(max(sizes))
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    d["pcm_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(x.stride(0))
    d["data_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    d["data_size"] = [round64(s) for s in sizes] if ring else sizes
    d["num_samples"] = [it.pcm.shape[0] for it in items]
    out = torch.full((n + 2, stride), IMG_FILL, dtype=torch.uint8, device="cuda")
    big = torch.from_numpy(guarded(input_records(items))).cuda()
    plan = engine.planar_encode_plan(param, d, x.stride(1), x.dtype)
    try:
        plan.run(x, out[1:n + 1], big[GUARD:GUARD + n * ch])
        torch.cuda.synchronize()
    finally:
        plan.close()
    host = out.cpu().numpy()
    assert (host[0] == IMG_FILL).all() and (host[n + 1] == IMG_FILL).all(), (label, "a row around the images was written")
    for i in range(n):
        assert (host[1 + i, int(d["data_size"][i]):] == IMG_FILL).all(), (label, "stream %d: a byte behind its data_size was written" % i)
    return [host[1 + i, :sizes[i]].tobytes() for i in range(n)], unguarded(label, big.cpu().numpy(), n * ch), None, None


def call_reconstruct(engine, torch, label, items, param, stats_only):
    """reconstruct_planar (int16 rows in, int16 rows + images + statistics out) / codec_error (from the float32 view)"""
    ch, n = param.num_channels, len(items)
    x = planar_x(torch, items, f32=stats_only)
    lens = [it.pcm.shape[0] for it in items]
    big = torch.from_numpy(guarded(input_records(items))).cuda()
    state = big[GUARD:GUARD + n * ch]
    if stats_only:
        stats = engine.codec_error(x, param, num_samples=lens, state=state)
        torch.cuda.synchronize()
        images, rows = None, None
    else:
        y, img, sizes, stats = engine.reconstruct_planar(x, param, num_samples=lens, dtype=torch.int16, state=state, return_images=True,
                                                         return_stats=True)
        torch.cuda.synchronize()
        host = img.cpu().numpy()
        images, rows = [host[i, :sizes[i]].tobytes() for i in range(n)], y.cpu().numpy()
    return images, unguarded(label, big.cpu().numpy(), n * ch), rows, stats.cpu().numpy()


def call_encode_host(engine, label, items, param):
    n = len(items) * param.num_channels
    big = guarded(input_records(items))
    state = big[GUARD:GUARD + n].view(LANE_STATE_DTYPE).reshape(-1)
    assert state.ctypes.data == big.ctypes.data + GUARD * 40
    images = engine.encode_host([it.pcm for it in items], param, state=state)
    return images, unguarded(label, big, n), None, None


def run_caller(engine, torch, caller, label, items, param, ring=False):
    if caller == "encode_plan":
        return call_encode_plan(engine, torch, label, items, param, ring)
    if caller == "encode_uniform":
        return call_encode_uniform(engine, torch, label, items, param)
    if caller.startswith("encode_planar"):
        return call_encode_planar(engine, torch, label, items, param, caller.endswith("f32"), ring)
    if caller in ("reconstruct_planar", "codec_error"):
        return call_reconstruct(engine, torch, label, items, param, caller == "codec_error")
    assert caller == "encode_host"
    return call_encode_host(engine, label, items, param)


def launch_sizes(caller, items):
    """streams per launch of a caller over the items of a group"""
    if caller != "encode_uniform":
        return [len(items)]
    return list(collections.Counter(it.pcm.shape[0] for it in items).values())


def every(it):
    return True


def check_group(engine, torch, policy, caller, mapping, lanes, key, members, corpus, ring=0, which=every):
    ch, bits, ms, trials, mbs = key
    items = permuted(members, corpus, seed=1000 * bits + 10 * ch + trials + mbs)
    param = make_parameter(ch, bits, mbs, 48000, ms, trials)
    rec = caller in ("reconstruct_planar", "codec_error")
    label = "%s, %s / %s%s, %dch %d-bit %s trials %d block %d" % (caller, mapping, lanes, ", byte ring" if ring == 2 else "", ch, bits,
                                                                 "M/S" if ms else "L/R", trials, mbs)
    kernel = None
    if caller != "encode_host":  # the plan first: a case must not claim a kernel it did not run
        kernel = claimed(mapping, lanes, ring, rec, ch, trials)
        for streams in launch_sizes(caller, items):
            got = policy(mapping, lanes, ring, rec, bits, ch, streams, trials, ob.geometry(mbs, ch, bits)[1])
            assert got == kernel, (label, streams, "planned", got, "claimed", kernel)
    images, records, rows, stats = run_caller(engine, torch, caller, label, items, param, ring == 2)
    assert engine.last_error() == "", (label, engine.last_error())
    if images is not None:
        check_images(label, images, items)
    check_records(label, records, items)
    pick = [i for i, it in enumerate(items) if which(it)]
    if rows is not None:
        check_rows(label, rows, items, which)
    if stats is not None:
        want = exact_stats(items)
        assert stats.dtype == np.int64 and np.array_equal(stats[pick], want[pick]), (
            label, "statistics differ from the sums over q(x) - decode of the image at [stream, channel, field]",
            [[pick[b[0]]] + b[1:].tolist() for b in np.argwhere(stats[pick] != want[pick])[:3]], "got", stats[pick].tolist(), "expected", want[pick].tolist())
    if which is every:
        TALLY[(caller, mapping, lanes if trials else "-", "ring" if ring == 2 else "", kernel or "(host tiles)")] += len(items)


@pytest.mark.parametrize("caller,mapping,lanes", RUNS, ids=["%s-%s-%s" % r for r in RUNS])
def test_state_callers(engine, corpus, policy, caller, mapping, lanes):
    """every format group of the corpus - all three tiers - through one caller under one mapping and trial-lane layout: images,
    every field of every output record, canaries, and for the reconstruct callers rows and exact statistics.  The pass over single
    trial lanes runs the groups with trials (without them it is the dual pass again)."""
    import torch
    engine.set_mapping(mapping, lanes)
    try:
        for key, members in groups().items():
            if lanes == "single" and key[3] == 0:
                continue
            check_group(engine, torch, policy, caller, mapping, lanes, key, members, corpus)
    finally:
        engine.set_mapping("auto", "dual")


@pytest.mark.parametrize("caller,mapping", [(c, m) for c in ("reconstruct_planar", "codec_error") for m in MAPPINGS])
def test_reconstruct_where_a_header_cannot_hold_the_weights(engine, corpus, policy, caller, mapping):
    """The regression test by name (module docstring): the groups with a stream whose decode is not the encoder's reconstruction -
    a wrapped header shift, INT32_MIN on a tap; mono, L/R, M/S and three channels - with the rows and statistics of those streams
    held to the oracle's decode of the golden image and the exact sums over q(x) - that decode."""
    import torch
    engine.set_mapping(mapping)
    ran, missed = 0, []
    try:
        for key, members in groups().items():
            if any(corpus[m["name"]].apart for m in members):
                ran += 1
                try:
                    check_group(engine, torch, policy, caller, mapping, "dual", key, members, corpus, which=lambda it: it.apart)
                except AssertionError as e:  # every group's figures, then fail
                    missed.append(str(e)[:700])
    finally:
        engine.set_mapping("auto")
    assert ran >= 7
    assert not missed, "\n".join(["%d of %d groups with such a stream miss the bar:" % (len(missed), ran)] + missed)


@pytest.mark.parametrize("caller", ["encode_plan", "encode_uniform", "encode_planar_i16", "encode_planar_f32"])
def test_state_through_the_byte_ring(ring_engine, corpus, policy, caller):
    """the dense encoders' byte ring (mono / stereo, no trials, images on 64-byte boundaries) starts from the carried record as
    well: its block header goes through the ring"""
    import torch
    ring_engine.set_mapping("dense")
    ran = 0
    for key, members in groups().items():
        if key[0] <= 2 and key[3] == 0:
            check_group(ring_engine, torch, policy, caller, "dense", "dual", key, members, corpus, ring=2)
            ran += 1
    assert ran == 6


@pytest.mark.parametrize("mapping", MAPPINGS)
def test_host_path_in_tiles(engine, corpus, policy, mapping):
    """encode_host with 1 KiB tiles: the groups are cut, so the caller's records enter the first tile (state_in), stay on the device
    between tiles (d_state) and come back after the last (state_back); then whole (tile size 0: built in)"""
    engine.set_mapping(mapping)
    try:
        for kbytes in (1, 0):
            engine.set_tile_kbytes(kbytes)
            for key, members in groups().items():
                check_group(engine, None, policy, "encode_host", mapping, "tiles %d" % kbytes, key, members, corpus)
    finally:
        engine.set_mapping("auto")
        engine.set_tile_kbytes(0)


@pytest.mark.parametrize("name", sorted(cs.SEQUENCES))
def test_legacy_handle_sequences(name):
    """the call sequences through AADEncoder_* of libaad_hip.so on ONE handle - bits, M/S, block size and channel count change
    between calls, some calls follow with no AADEncoder_SetEncodeParameter (the index carried), some are 1 .. 5 samples long -
    against the compiled reference's image hashes (every image after the first depends on the state the handle kept)"""
    lib = aad_amd.load_library()
    calls = cs.SEQUENCES[name]
    want = cs.golden()["sequences"][name]
    oracle = cs.oracle_sequence(calls)
    for k, image in enumerate(cs.api_sequence(lib, calls)):
        assert sha256(oracle[k][1]) == want[k]["image_sha256"], (name, k)
        assert image == oracle[k][1], cp.describe_mismatch("sequence %s call %d %s" % (name, k, calls[k]), image, oracle[k][1])


def test_parameter_change_on_a_device_state_tensor(engine):
    """One state tensor through four calls that change the format: 2-bit L/R, 4-bit M/S with trials on the same records, mono 3-bit
    on channel 0's records (re-packed by the test, channel 1's kept), 3-bit L/R on both again with the index carried.  Each
    call's images and the records after it == the oracle's on lanes carried the same way."""
    import torch
    streams = 5
    starts = [["shift13", "min32768"], ["reached_tone_music/0", "reached_tone_music/1"], ["zero", "shift15_top"], ["idx4080", "idx0"],
              ["alternating", "max32767"]]
    lanes = [cs.lanes_of([cs.record(n) for n in names], i) for i, names in enumerate(starts)]
    state = np.zeros(streams * 2, dtype=LANE_STATE_DTYPE)
    for i, names in enumerate(starts):
        for c, n in enumerate(names):
            r = cs.record(n)
            state[2 * i + c] = (r["w"], cs.garbage_history(i, c), r["idx"], r["qerr"])
    big = torch.from_numpy(guarded(state)).cuda()
    table = big[GUARD:GUARD + 2 * streams]
    # (channels, bits, ms, trials, max_block_size, frames, family, the index reset in front of the call)
    calls = [(2, 2, False, 0, 128, None, "tone_p6", False), (2, 4, True, 2, 1024, 700, "rail_stereo", True),
             (1, 3, False, 1, 60, 333, "saw", True), (2, 3, False, 0, 256, None, "square_p128", False)]
    for k, (ch, bits, ms, trials, mbs, frames, family, reset) in enumerate(calls):
        frames = 2 * ob.geometry(mbs, ch, bits)[2] + 19 if frames is None else frames
        param = make_parameter(ch, bits, mbs, 48000, ms, trials)
        pcm = np.stack([cp.generate(family, frames, ch, i % 2) for i in range(streams)])
        pcm[:, :, 0] += np.arange(streams, dtype=np.int16)[:, None] * (0 if family == "rail_stereo" else 1)  # streams differ
        if reset:
            table[:, 8] = 0
        if ch == 2:
            d_img, size = engine.encode_uniform(torch.from_numpy(pcm).cuda(), param, state=table)
        else:  # the mono call: channel 0's records packed into a table of their own, written back behind the call
            mono = table.view(streams, 2, 10)[:, 0].contiguous()
            d_img, size = engine.encode_uniform(torch.from_numpy(pcm).cuda(), param, state=mono)
            table.view(streams, 2, 10)[:, 0] = mono
        torch.cuda.synchronize()
        host = d_img.cpu().numpy()
        got = unguarded("call %d" % k, big.cpu().numpy(), 2 * streams)
        for i in range(streams):
            if reset:
                for l in lanes[i]:
                    l.idx = 0
            want = ob.encode(pcm[i], bits, mbs, 48000, ms, trials, lanes=lanes[i], reset_idx=False)
            assert host[i, :size].tobytes() == want, cp.describe_mismatch("call %d stream %d" % (k, i), host[i, :size].tobytes(), want)
            for c, w in enumerate(cs.lanes_out(lanes[i])):
                r = got[2 * i + c]
                have = {"w": [int(v) for v in r["weight"]], "h": [int(v) for v in r["history"]], "idx": int(r["stepsize_index"]),
                        "qerr": int(r["quantize_error"])}
                # both channels' records after every call: the mono call leaves channel 1's as they were, in the oracle and here
                assert have == w, ("call %d stream %d channel %d" % (k, i, c), have, w)


def test_segmented_plans_take_no_state(engine):
    """segmented encodes start from fresh encoders: a state table with one is refused, by the engine and by the C ABI"""
    import torch
    from aad_amd.capi import AADApiResult
    param = make_parameter(1, 4, 128, 48000, False, 0)
    d_pcm = torch.from_numpy(np.stack([cp.generate("saw", 1500, 1, v) for v in range(2)])).cuda()
    state = torch.zeros((2, 10), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        engine.encode_uniform(d_pcm, param, state=state, segment_blocks=2)
    plan = engine.uniform_encode_plan(param, 2, 1500, segment_blocks=2, warmup_blocks=1)
    try:
        data = torch.zeros((2, plan.stride), dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError):
            plan.run(d_pcm, data, state)
        assert engine.lib.AADHip_EncodePlanRun(plan.handle, d_pcm.data_ptr(), data.data_ptr(), state.data_ptr()) == AADApiResult.INVALID_ARGUMENT
    finally:
        plan.close()
    assert not state.cpu().numpy().any()


def test_zz_what_ran(capsys):
    """prints the cases compared per caller, mapping, trial lanes and kernel the policy named (run last: -s or the captured output)"""
    with capsys.disabled():
        print("\ncaller mapping lanes ring kernel cases")
        for key, count in sorted(TALLY.items()):
            print(" ".join(str(k) if k != "" else "-" for k in key), count)
