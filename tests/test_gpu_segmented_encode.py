"""Segmented encode plans (AADHip_SegmentedEncodePlanCreate) on the GPU: the images equal the definition's bytes
(tests/segment_oracle.py, the oracle run on the slices) for every geometry, trial count, lane mapping and trial-lane setting,
segment length and warm-up; both mapping regimes run; no store leaves a stream's image; a stream's bytes do not depend on the
batch around it; the reference decoder reads the images; the refusals.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import AADApiResult, AADHipSegmentation, ApiError, STREAM_DESC_DTYPE, make_parameter
from aad_amd.synth import synth_pcm

pytestmark = pytest.mark.gpu

CANARY = 0xA5
MBS = 256
MAPPINGS = ["auto", "dense", "quad", "quad-fused", "dense-tiled"]
# (channels, M/S)
LAYOUTS = [(1, False), (2, False), (2, True), (8, False)]


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401  (loads the HIP runtime the library then shares)
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_mapping("auto", "dual")
    e.close()


def spb_of(ch, bits, mbs=MBS):
    return ob.geometry(mbs, ch, bits)[2]


def run_batch(engine, param, pcms, L, W, lead=3, gap=13):
    """Encode pcms (int16 [frames, ch] each) as ONE segmented plan.  Images at odd offsets (lead, then gap canary bytes between and
    after them); every canary byte must survive.  -> list of images (bytes)."""
    import torch
    sizes = [engine.encoded_size(param, p.shape[0]) for p in pcms]
    d = np.zeros(len(pcms), dtype=STREAM_DESC_DTYPE)
    off, pcm_off = lead, 0
    for i, p in enumerate(pcms):
        d[i] = (pcm_off, off, sizes[i], p.shape[0], 0)
        off += sizes[i] + gap
        pcm_off += p.size
    total = off
    flat = np.concatenate([p.reshape(-1) for p in pcms]).astype(np.int16)
    d_pcm = torch.from_numpy(flat).cuda()
    d_out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    plan = engine.encode_plan(param, d, L, W)
    try:
        plan.run(d_pcm, d_out)
        torch.cuda.synchronize()
    finally:
        plan.close()
    out = d_out.cpu().numpy()
    images, mask = [], np.ones(total, dtype=bool)
    for i in range(len(pcms)):
        o = int(d["data_offset"][i])
        images.append(out[o:o + sizes[i]].tobytes())
        mask[o:o + sizes[i]] = False
    bad = np.nonzero(out[mask] != CANARY)[0]
    assert bad.size == 0, "%d canary bytes changed (L=%d W=%d), first at %s" % (bad.size, L, W, np.nonzero(mask)[0][bad[:4]])
    return images


def ragged(ch, bits, seed, long_blocks=300):
    """a 1-frame stream, a one-block stream and a long one ending in a short block"""
    spb = spb_of(ch, bits)
    lens = [1, spb, long_blocks * spb - spb // 3]
    return [synth_pcm(1, n, ch, seed=seed + i)[0] for i, n in enumerate(lens)]


@pytest.mark.parametrize("trials", [0, 1, 2])
@pytest.mark.parametrize("ch,ms", LAYOUTS, ids=["mono", "lr", "ms", "ch8"])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_bit_exact_against_the_definition(engine, bits, ch, ms, trials):
    pcms = ragged(ch, bits, seed=100 * bits + 10 * ch + trials, long_blocks=300 if ch < 8 else 60)
    B = -(-pcms[-1].shape[0] // spb_of(ch, bits))
    param = make_parameter(ch, bits, MBS, 48000, ms, trials)
    cases = [(1, 0), (2, 1), (7, 3), (7, 0), (1, 10 ** 6), (B, 0), (B + 4, 2)]
    want = {lw: [so.segmented_encode(p, bits, lw[0], lw[1], MBS, ms=ms, trials=trials) for p in pcms] for lw in cases}
    serial = [ob.encode(p, bits, MBS, 48000, ms, trials) for p in pcms]
    assert want[(B, 0)] == serial and want[(1, 10 ** 6)] == serial
    lanes = ["dual", "single"] if trials else ["dual"]
    for mapping in MAPPINGS:
        for tl in lanes:
            engine.set_mapping(mapping, tl)
            for L, W in cases:
                got = run_batch(engine, param, pcms, L, W)
                for i, (g, w) in enumerate(zip(got, want[(L, W)])):
                    assert g == w, "stream %d differs: mapping=%s trial_lanes=%s L=%d W=%d" % (i, mapping, tl, L, W)
    engine.set_mapping("auto", "dual")


@pytest.mark.parametrize("trials", [0, 2])
@pytest.mark.parametrize("chains", [16384, 16385, 20000])
def test_both_mapping_regimes(engine, chains, trials):
    """mono chains: up to 16 384 recurrences `auto` takes the quad encoder, beyond it the dense one"""
    engine.set_mapping("auto", "dual")
    bits, ch = 4, 1
    spb = spb_of(ch, bits)
    L, W = 2, 1
    pcm = synth_pcm(1, chains * L * spb - 5, ch, seed=chains + trials)[0]
    param = make_parameter(ch, bits, MBS, 48000, False, trials)
    got = run_batch(engine, param, [pcm], L, W)[0]
    assert got == so.segmented_encode(pcm, bits, L, W, MBS, trials=trials)


def test_containment_at_odd_offsets(engine):
    """stereo 4-bit (the dense burst stores and their deferred bytes) with images at every offset mod 64, chain ends in the
    middle of 64-byte sectors: nothing outside the images changes, the bytes are the definition's"""
    bits, ch = 4, 2
    spb = spb_of(ch, bits)
    pcms = [synth_pcm(1, n, ch, seed=7 + n)[0] for n in (spb * 9 + 1, spb * 4, 3, spb * 11 - 2)]
    for mapping in ("dense", "quad"):
        engine.set_mapping(mapping, "dual")
        for lead, gap in ((1, 1), (3, 61), (63, 2), (64, 64), (17, 5)):
            for L, W in ((1, 1), (3, 2)):
                got = run_batch(engine, make_parameter(ch, bits, MBS), pcms, L, W, lead=lead, gap=gap)
                assert got == [so.segmented_encode(p, bits, L, W, MBS) for p in pcms], (mapping, lead, gap, L, W)
    engine.set_mapping("auto", "dual")


@pytest.mark.parametrize("trials", [0, 2])
def test_batch_independence(engine, trials):
    bits, ch = 4, 2
    spb = spb_of(ch, bits)
    param = make_parameter(ch, bits, MBS, 48000, False, trials)
    mine = synth_pcm(1, spb * 23 - 7, ch, seed=99)[0]
    others = [synth_pcm(1, n, ch, seed=n)[0] for n in (1, spb, spb * 40, spb * 5 + 3)]
    L, W = 4, 2
    alone = run_batch(engine, param, [mine], L, W)[0]
    assert alone == so.segmented_encode(mine, bits, L, W, MBS, trials=trials)
    for pos in (0, 2, len(others)):
        batch = others[:pos] + [mine] + others[pos:]
        assert run_batch(engine, param, batch, L, W, lead=5 + pos)[pos] == alone, pos


@pytest.mark.ref
@pytest.mark.parametrize("bits,ch,trials", [(4, 2, 0), (4, 2, 2), (3, 1, 1), (2, 2, 0)])
def test_reference_decoder_reads_the_images(engine, bits, ch, trials):
    param = make_parameter(ch, bits, MBS, 48000, False, trials)
    pcms = ragged(ch, bits, seed=3, long_blocks=120)
    images = run_batch(engine, param, pcms, 5, 2)
    ours = engine.decode_host(images)
    for p, img, dec in zip(pcms, images, ours):
        theirs = so.ref_decode(img, p.shape[0], ch)
        assert np.array_equal(np.asarray(dec).reshape(theirs.shape), theirs)
        assert np.array_equal(theirs, ob.decode(img)[0])


def test_python_surface_and_refusals(engine):
    import torch
    bits, ch = 4, 2
    spb = spb_of(ch, bits, 1024)
    pcm = synth_pcm(4, spb * 9 + 5, ch, seed=21)
    param = make_parameter(ch, bits, 1024)
    d_pcm = torch.from_numpy(pcm).cuda()
    out, size = engine.encode_uniform(d_pcm, param, segment_blocks=2, warmup_blocks=1)
    torch.cuda.synchronize()
    img = out.cpu().numpy()
    for s in range(4):
        assert img[s, :size].tobytes() == so.segmented_encode(pcm[s], bits, 2, 1, 1024)
    # the plain path is untouched
    out0, size0 = engine.encode_uniform(d_pcm, param)
    torch.cuda.synchronize()
    assert size0 == size and out0.cpu().numpy()[0, :size].tobytes() == ob.encode(pcm[0], bits, 1024)

    state = torch.zeros((4 * ch, 10), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        engine.encode_uniform(d_pcm, param, state=state, segment_blocks=2)
    with pytest.raises(ApiError) as e:
        engine.encode_uniform(d_pcm, param, segment_blocks=0)
    assert e.value.code == AADApiResult.INVALID_ARGUMENT

    plan = engine.uniform_encode_plan(param, 4, pcm.shape[1], segment_blocks=3, warmup_blocks=1)
    data = torch.zeros((4, plan.stride), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        plan.run(d_pcm, data, state)
    # the C ABI itself: device_state on a segmented plan, a null segmentation
    lib = engine.lib
    rc = lib.AADHip_EncodePlanRun(plan.handle, d_pcm.data_ptr(), data.data_ptr(), state.data_ptr())
    assert rc == AADApiResult.INVALID_ARGUMENT
    plan.run(d_pcm, data)
    torch.cuda.synchronize()
    assert data.cpu().numpy()[1, :plan.image_size].tobytes() == so.segmented_encode(pcm[1], bits, 3, 1, 1024)
    plan.close()
    h = C.c_void_p()
    rc = lib.AADHip_SegmentedEncodePlanCreate(engine._ctx, C.byref(param), None, 4, plan.descs.ctypes.data, C.byref(h))
    assert rc == AADApiResult.INVALID_ARGUMENT and not h.value
    seg = AADHipSegmentation(0, 4)
    rc = lib.AADHip_SegmentedEncodePlanCreate(engine._ctx, C.byref(param), C.byref(seg), 4, plan.descs.ctypes.data, C.byref(h))
    assert rc == AADApiResult.INVALID_ARGUMENT and not h.value
    # validation as AADHip_EncodePlanCreate: a capacity one byte short
    short = plan.descs.copy()
    short["data_size"][2] = plan.image_size - 1
    seg = AADHipSegmentation(2, 1)
    rc = lib.AADHip_SegmentedEncodePlanCreate(engine._ctx, C.byref(param), C.byref(seg), 4, short.ctypes.data, C.byref(h))
    assert rc == AADApiResult.INSUFFICIENT_BUFFER == lib.AADHip_EncodePlanCreate(engine._ctx, C.byref(param), 4,
                                                                                  short.ctypes.data, C.byref(h))
