"""GPU parity on the crafted-PCM corpus (tests/crafted_pcm.py): every encoder and decoder kernel through the corners the three
synthetic kinds never reach - block headers with a weight shift of 2 .. 13 (weights near 2^28: every h*w product and the prediction
sum wrap int32), both clip rails for whole blocks, the step index resting at 0 or crossing its whole range inside a block.

The expected value is always the oracle's bytes (oracle_binding.encode / decode).  tests/test_crafted_pcm.py pins those to the
compiled reference; here - where the reference does not exist - the `corpus` fixture first checks them against the reference's
hashes in tests/golden/crafted_pcm.json.  Bar: bit-exact images and PCM; statistics as in tests/test_gpu_planar_stats.py (== on
integers) and tests/test_gpu_reconstruct.py (1e-12 relative on the reordered fp64 sums, == on the maximum and the printed line).

Which kernel a single chain takes (aad_launch_policy.h plan_encode / plan_decode; one mono stream = one recurrence):
  encode  auto        Quad (one recurrence is far below the 16 384 where "auto" turns dense); with trials QuadDual
          dense       Dense, one-wave workgroup, per-lane stores (the byte ring needs four-wave workgroups: see the ring test)
          dense-tiled Dense (the option only concerns the decoder)
          quad        Quad; with trials QuadDual (trial lanes "dual", the default)
          quad-fused  Quad / QuadDual (the option only concerns the decoder)
  decode  (87 - 174 blocks = that many recurrences: every block header carries the whole state)
          auto, quad  SplitLds for the mono 4-bit cases (2012 coded samples a block <= kLdsResidualMax), SplitScratch for the others
          quad-fused  QuadFused
          dense       Dense
          dense-tiled Tiled for mono 4- and 2-bit (the 2-bit block's 8056 PCM bytes take the odd-8 lead chunk); mono 3-bit blocks of
                      2684 samples are 8 mod 16 bytes long and take Dense, as do the stereo case's 2-bit blocks under "auto".
A failing assertion names the case, the mapping, the first differing block and that block's header fields from both sides."""
import numpy as np
import pytest

import crafted_pcm as cp
import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import STREAM_DESC_DTYPE, make_parameter
from helpers import sha256
from test_oracle_golden import extract_channel_as_mono
from window_oracle import window_expected

pytestmark = pytest.mark.gpu

MAPPINGS = ["auto", "dense", "dense-tiled", "quad", "quad-fused"]
STATS_RTOL = 1e-12  # tests/test_gpu_reconstruct.py
LONG = cp.long_cases()
SHORT = cp.short_cases()
LONG_2BIT = [c for c in LONG if c["bits"] == 2 and c["trials"] == 0 and c["channels"] == 1][0]
LONG_STEREO = [c for c in LONG if c["channels"] == 2][0]
# a dozen short cases for the device-resident paths: every family, 1 / 2 / 3 / 8 channels, M/S, trials 0 and 2
_POOL = [c for c in SHORT if (c["bits"], c["trials"]) in ((2, 0), (4, 2))]
DOZEN = _POOL[::2] + _POOL[1:2]
assert len(DOZEN) == 12


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus():
    """{name: (case, pcm, oracle image, oracle decode)}, computed once; the oracle's results checked against the reference's hashes"""
    golden = cp.golden()
    out = {}
    for c in cp.cases():
        rec = golden[c["name"]]
        pcm = cp.case_pcm(c)
        assert sha256(pcm.tobytes()) == rec["pcm_sha256"], c["name"]
        image = cp.oracle_encode(c, pcm)
        decoded = ob.decode(image)[0]
        if c["channels"] <= 2:
            assert sha256(image) == rec["image_sha256"] and sha256(decoded.tobytes()) == rec["decoded_sha256"], c["name"]
        else:
            for ch in range(c["channels"]):
                assert sha256(extract_channel_as_mono(image, ch, rec["mono_block_size"])) == rec["mono_image_sha256"][ch], c["name"]
                assert sha256(np.ascontiguousarray(decoded[:, ch]).tobytes()) == rec["mono_decoded_sha256"][ch], c["name"]
        out[c["name"]] = (c, pcm, image, decoded)
    return out


def param_of(c):
    return make_parameter(c["channels"], c["bits"], c["max_block_size"], 48000, c["ms"], c["trials"])


def check_image(label, got, want):
    assert bytes(got) == want, cp.describe_mismatch(label, got, want)


def check_pcm(label, got, want, image):
    assert np.array_equal(got, want), cp.describe_pcm_mismatch(label, got, want, image)


def plan_encode(engine, pcms, param):
    """a ragged device-resident encode plan with every image on a 64-byte boundary (the layout the byte ring takes) -> list of bytes"""
    import torch
    ch = param.num_channels
    d = np.zeros(len(pcms), dtype=STREAM_DESC_DTYPE)
    pos_p = pos_d = 0
    sizes = []
    for i, p in enumerate(pcms):
        size = engine.encoded_size(param, p.shape[0])
        sizes.append(size)
        d["pcm_offset"][i], d["data_offset"][i], d["data_size"][i], d["num_samples"][i] = pos_p, pos_d, -(-size // 64) * 64, p.shape[0]
        pos_p += p.shape[0] * ch
        pos_d += -(-size // 64) * 64
    d_pcm = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pcms])).cuda()
    d_img = torch.zeros(pos_d, dtype=torch.uint8, device="cuda")
    plan = engine.encode_plan(param, d)
    try:
        plan.run(d_pcm, d_img, None)
        torch.cuda.synchronize()
    finally:
        plan.close()
    img = d_img.cpu().numpy()
    return [img[int(d["data_offset"][i]):int(d["data_offset"][i]) + sizes[i]].tobytes() for i in range(len(pcms))]


# ---- short cases: host batches under every mapping, whole and in 64 KiB tiles --------------------------------------------------------

@pytest.mark.parametrize("tile_kbytes", [0, 64])
@pytest.mark.parametrize("mapping", MAPPINGS)
def test_short_cases_host_batches(engine, corpus, mapping, tile_kbytes):
    groups = {}
    for c in SHORT:
        groups.setdefault((c["channels"], c["bits"], c["ms"], c["trials"], c["max_block_size"]), []).append(c)
    engine.set_mapping(mapping)
    engine.set_tile_kbytes(tile_kbytes)
    try:
        for key, members in sorted(groups.items()):
            pcms = [corpus[c["name"]][1] for c in members]
            images = engine.encode_host(pcms, param_of(members[0]))
            for c, img in zip(members, images):
                check_image("%s, encode %s, tiles %d" % (c["name"], mapping, tile_kbytes), img, corpus[c["name"]][2])
            decoded = engine.decode_host([corpus[c["name"]][2] for c in members])
            for c, d in zip(members, decoded):
                check_pcm("%s, decode %s, tiles %d" % (c["name"], mapping, tile_kbytes), d, corpus[c["name"]][3], corpus[c["name"]][2])
    finally:
        engine.set_mapping("auto")
        engine.set_tile_kbytes(0)


# ---- long cases: one chain alone, and batched with 63 short streams ----------------------------------------------------------------

@pytest.mark.parametrize("case", LONG, ids=[c["name"] for c in LONG])
def test_long_case_alone_every_mapping(engine, corpus, case):
    """a single chain under every mapping (the kernels: module docstring), whole and - the decoders - in 64 KiB tiles"""
    _, pcm, want, decoded = corpus[case["name"]]
    try:
        for mapping in MAPPINGS:
            engine.set_mapping(mapping)
            check_image("%s alone, encode %s" % (case["name"], mapping), engine.encode_host([pcm], param_of(case))[0], want)
            for tile in (0, 64):
                engine.set_tile_kbytes(tile)
                check_pcm("%s alone, decode %s, tiles %d" % (case["name"], mapping, tile), engine.decode_host([want])[0], decoded, want)
            engine.set_tile_kbytes(0)
    finally:
        engine.set_mapping("auto")
        engine.set_tile_kbytes(0)


@pytest.mark.parametrize("case", LONG[:6], ids=[c["name"] for c in LONG[:6]])
def test_long_case_batched_with_63_short(engine, corpus, case, monkeypatch):
    """The long chain as stream 5 of 64 mono streams: the dense bodies run it inside a full wave whose other lanes finish early, the
    trial search with neighbours, and - trials 0, on a context with AAD_HIP_ENCODE_RING=2, images on 64-byte boundaries - the dense
    encoder's byte ring.  Host batches whole and in tiles; decode under every mapping."""
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    _, pcm, want_long, _ = corpus[case["name"]]
    pcms = cp.companions(case["bits"])
    pcms.insert(5, pcm)
    want = [want_long if i == 5 else ob.encode(p, case["bits"], 1024, 48000, False, case["trials"]) for i, p in enumerate(pcms)]
    decoded = [ob.decode(w)[0] for w in want]
    param = param_of(case)
    try:
        for mapping, tile in (("dense", 0), ("dense", 64), ("auto", 0), ("quad", 64)):
            engine.set_mapping(mapping)
            engine.set_tile_kbytes(tile)
            for i, img in enumerate(engine.encode_host(pcms, param)):
                check_image("%s batched (stream %d of 64), encode %s, tiles %d" % (case["name"], i, mapping, tile), img, want[i])
        engine.set_tile_kbytes(0)
        for mapping in MAPPINGS:
            engine.set_mapping(mapping)
            for i, d in enumerate(engine.decode_host(want)):
                check_pcm("%s batched (stream %d of 64), decode %s" % (case["name"], i, mapping), d, decoded[i], want[i])
        engine.set_mapping("dense")
        for i, img in enumerate(plan_encode(engine, pcms, param)):
            check_image("%s batched (stream %d of 64), device plan, dense" % (case["name"], i), img, want[i])
    finally:
        engine.set_mapping("auto")
        engine.set_tile_kbytes(0)
    if case["trials"] == 0:
        monkeypatch.setenv("AAD_HIP_ENCODE_RING", "2")  # read when a context is created
        ring = Engine(0)
        try:
            ring.set_mapping("dense")
            for i, img in enumerate(plan_encode(ring, pcms, param)):
                check_image("%s batched (stream %d of 64), device plan, dense with the byte ring" % (case["name"], i), img, want[i])
        finally:
            ring.close()


# ---- device-resident paths ---------------------------------------------------------------------------------------------------------

def exact_stats(x, y):
    """int64 [C, 4] (sum_sq, sum_abs, max_abs, count) of x - y, int16 [n, C] each: python integers from int64 columns (|e| < 2^16, so
    e^2 < 2^32 and 350 436 of them stay far below 2^63)"""
    e = x.astype(np.int64) - y.astype(np.int64)
    return np.array([[int((e[:, c] * e[:, c]).sum()), int(np.abs(e[:, c]).sum()), int(np.abs(e[:, c]).max()), e.shape[0]]
                     for c in range(e.shape[1])], dtype=np.int64)


SUBJECTS = [LONG_2BIT, LONG_STEREO] + DOZEN


@pytest.mark.parametrize("case", SUBJECTS, ids=[c["name"] for c in SUBJECTS])
def test_device_resident_paths(engine, corpus, case):
    """encode_uniform / decode_uniform, planar encode from int16 and float32 rows, planar reconstruct with its exact statistics, and
    the host reconstruct modes, each against the oracle.  On the long 2-bit tone the codec has lost the signal (maximum error about
    28 000 - 60 000 after the weights diverge), so the sums are large: sum_sq of the order of 10^14."""
    import torch
    _, pcm, want, decoded = corpus[case["name"]]
    name, param = case["name"], param_of(case)
    d_pcm = torch.from_numpy(pcm[None]).cuda()
    d_img, size = engine.encode_uniform(d_pcm, param)
    d_dec, _ = engine.decode_uniform(d_img, size)
    torch.cuda.synchronize()
    check_image(name + ", encode_uniform", d_img[0, :size].cpu().numpy(), want)
    check_pcm(name + ", decode_uniform", d_dec[0].cpu().numpy(), decoded, want)
    # planar rows [1, C, T]: the same image from int16 and from float32 (x / 32768 is exact)
    rows = torch.from_numpy(np.ascontiguousarray(pcm.T)[None]).cuda()
    for x in (rows, rows.to(torch.float32) / 32768.0):
        p_img, sizes = engine.encode_planar(x, param)
        torch.cuda.synchronize()
        assert sizes == [len(want)]
        check_image("%s, encode_planar from %s" % (name, x.dtype), p_img[0, :sizes[0]].cpu().numpy(), want)
        y, stats = engine.reconstruct_planar(x, param, dtype=torch.int16, return_stats=True)
        torch.cuda.synchronize()
        check_pcm("%s, reconstruct_planar from %s" % (name, x.dtype), y[0].cpu().numpy().T, decoded, want)
        got, exact = stats[0].cpu().numpy(), exact_stats(pcm, decoded)
        assert np.array_equal(got, exact), (name, str(x.dtype), "planar statistics", got.tolist(), exact.tolist())
    # the reference CLI's reconstruction modes through the host entry point
    rec, st = engine.reconstruct_host([pcm], param, residual=False)
    gap, st_g = engine.reconstruct_host([pcm], param, residual=True)
    check_pcm(name + ", reconstruct_host", rec[0], decoded, want)
    assert np.array_equal(gap[0], ob.residual(pcm, decoded)), name
    want_stats = ob.error_stats(pcm, decoded)
    for s in (st[0], st_g[0]):
        got = (float(s["rms_error"]), float(s["mean_abs_error"]), float(s["max_abs_error"]))
        np.testing.assert_allclose(got, want_stats, rtol=STATS_RTOL, atol=0, err_msg=name)
        assert got[2] == want_stats[2] and ob.stats_line(got) == ob.stats_line(want_stats), (name, got, want_stats)


def test_long_2bit_error_is_as_large_as_claimed(corpus):
    """the docstring's magnitudes, from the oracle alone: the diverged 2-bit chain's maximum error"""
    _, pcm, _, decoded = corpus[LONG_2BIT["name"]]
    stats = exact_stats(pcm, decoded)
    assert 28000 <= stats[0, 2] <= 65535 and stats[0, 0] > 10 ** 13


@pytest.mark.parametrize("case", LONG, ids=[c["name"] for c in LONG])
def test_window_decode_around_the_diverged_blocks(engine, corpus, case):
    """windows before, across and after the first block whose header shift reaches 8 (where the case gets there; else 2; the
    control: mid-stream), at block starts and mid-block, int16 and float32, against slices of the oracle's decode"""
    import torch
    _, pcm, want, decoded = corpus[case["name"]]
    spb = ob.geometry(case["max_block_size"], case["channels"], case["bits"])[2]
    blocks = -(-len(pcm) // spb)
    b = cp.first_block_with_shift(want, 8) or cp.first_block_with_shift(want, 2) or blocks // 2
    d_img = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()[None]).cuda()
    for frames in (100, spb + 77):
        firsts = [0, (b - 2) * spb + 5, b * spb - 50, b * spb - frames // 2, b * spb, b * spb + 1, (b + 1) * spb - 3, (b + 9) * spb + 11,
                  (blocks - 1) * spb - 40, len(pcm) - frames // 3]
        windows = np.array([(0, f) for f in firsts], dtype=np.int64)
        expected = window_expected([decoded], windows, frames, case["channels"])
        got16 = engine.decode_windows(d_img, len(want), torch.from_numpy(windows).cuda(), frames, torch.int16).cpu().numpy()
        for w, f in enumerate(firsts):
            assert np.array_equal(got16[w], expected[w]), cp.describe_pcm_mismatch(
                "%s, window of %d frames at %d" % (case["name"], frames, f), got16[w].T, expected[w].T)
        got32 = engine.decode_windows(d_img, len(want), torch.from_numpy(windows).cuda(), frames, torch.float32).cpu().numpy()
        want32 = expected.astype(np.float32) / np.float32(32768.0)
        assert np.array_equal(got32.view(np.uint32), want32.view(np.uint32)), (case["name"], frames, "float32 is not int16 / 32768")


@pytest.mark.parametrize("segment_blocks,warmup_blocks", [(16, 4), (64, 8)])
def test_segmented_encode_of_the_long_2bit_case(engine, corpus, segment_blocks, warmup_blocks):
    """Every segment starts from zero weights behind its warm-up blocks, so the image is another stream than the chain's - the
    definition (tests/segment_oracle.py) decides: bytes equal to it, and the image decodes the same on the device and in the oracle."""
    import torch
    case = LONG_2BIT
    _, pcm, chain, _ = corpus[case["name"]]
    want = so.segmented_encode(pcm, case["bits"], segment_blocks, warmup_blocks, case["max_block_size"])
    assert len(want) == len(chain) and want != chain
    d_img, size = engine.encode_uniform(torch.from_numpy(pcm[None]).cuda(), param_of(case), segment_blocks=segment_blocks,
                                        warmup_blocks=warmup_blocks)
    d_dec, _ = engine.decode_uniform(d_img, size)
    torch.cuda.synchronize()
    label = "%s, segmented encode (%d, %d)" % (case["name"], segment_blocks, warmup_blocks)
    check_image(label, d_img[0, :size].cpu().numpy(), want)
    check_pcm(label + ", decode_uniform", d_dec[0].cpu().numpy(), ob.decode(want)[0], want)
    print("\n%s: largest header shift %d (the chain: %d)" % (label, cp.max_header_shift(want), cp.max_header_shift(chain)))
