"""Segmented encode from host memory and the reconstruction modes over segmented images, on the GPU:
AADHip_SegmentedEncodeBatch, AADHip_SegmentedReconstructPlanCreate, AADHip_SegmentedReconstructBatch, aad_batch -S and the Python
surfaces.  Expected bytes come from tests/segment_oracle.py (the definition in include/aad_hip.h, pinned to the oracle and the
compiled reference); the reconstructions are checked against the oracle's decode of those bytes.  Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import AADApiResult, AADHipSegmentation, ApiError, STREAM_DESC_DTYPE, make_parameter
from aad_amd.synth import synth_pcm
from helpers import ROOT, read_wav16, wav16_bytes

pytestmark = pytest.mark.gpu

MBS = 256
CLI = os.path.join(ROOT, "aad_amd", "aad_batch")
# (channels, M/S)
LAYOUTS = [(1, False), (2, False), (2, True), (8, False)]


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401  (loads the HIP runtime the library then shares)
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_tile_kbytes(0)
    e.set_compare_order(sequential=False)
    e.close()


def spb_of(ch, bits, mbs=MBS):
    return ob.geometry(mbs, ch, bits)[2]


def want_images(pcms, bits, L, W, mbs=MBS, ms=False, trials=0):
    return [so.segmented_encode(p, bits, L, W, mbs, ms=ms, trials=trials) for p in pcms]


def plan_images(engine, param, pcms, L, W):
    """the device-resident segmented plan (AADHip_SegmentedEncodePlanCreate + AADHip_EncodePlanRun) on copies of pcms"""
    import torch
    sizes = [engine.encoded_size(param, p.shape[0]) for p in pcms]
    d = np.zeros(len(pcms), dtype=STREAM_DESC_DTYPE)
    off, pcm_off = 0, 0
    for i, p in enumerate(pcms):
        d[i] = (pcm_off, off, sizes[i], p.shape[0], 0)
        off += sizes[i] + 5
        pcm_off += p.size
    d_pcm = torch.from_numpy(np.concatenate([p.reshape(-1) for p in pcms]).astype(np.int16)).cuda()
    d_out = torch.zeros(off, dtype=torch.uint8, device="cuda")
    plan = engine.encode_plan(param, d, L, W)
    try:
        plan.run(d_pcm, d_out)
        torch.cuda.synchronize()
    finally:
        plan.close()
    out = d_out.cpu().numpy()
    return [out[int(d["data_offset"][i]):int(d["data_offset"][i]) + sizes[i]].tobytes() for i in range(len(pcms))]


def ragged(ch, bits, seed, long_blocks):
    """a 1-frame stream, one shorter than a block, a one-block stream and a long one ending in a short block"""
    spb = spb_of(ch, bits)
    lens = [1, spb // 2 + 1, spb, long_blocks * spb - spb // 3]
    return [synth_pcm(1, n, ch, seed=seed + i)[0] for i, n in enumerate(lens)]


@pytest.mark.parametrize("trials", [0, 2, 255])
@pytest.mark.parametrize("ch,ms", LAYOUTS, ids=["mono", "lr", "ms", "ch8"])
@pytest.mark.parametrize("bits", [2, 3, 4])
def test_encode_batch_equals_the_definition(engine, bits, ch, ms, trials):
    long_blocks = 40 if trials == 255 else (50 if ch == 8 else 120)
    pcms = ragged(ch, bits, seed=1000 + 100 * bits + 10 * ch + trials % 7, long_blocks=long_blocks)
    B = -(-pcms[-1].shape[0] // spb_of(ch, bits))
    param = make_parameter(ch, bits, MBS, 48000, ms, trials)
    # W > s L (the warm-up clamped at the stream's start), L >= B (the reference's bytes), W = 0, L = 1
    cases = [(3, 5), (7, 2), (1, 0), (B, 0), (B + 3, 4), (16, 4)]
    for L, W in cases:
        want = want_images(pcms, bits, L, W, ms=ms, trials=trials)
        got = engine.encode_host(pcms, param, segment_blocks=L, warmup_blocks=W)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "stream %d (%d frames) differs: L=%d W=%d" % (i, pcms[i].shape[0], L, W)
        if L >= B:
            assert got == [ob.encode(p, bits, MBS, 48000, ms, trials) for p in pcms]


@pytest.mark.parametrize("tile_kbytes", [1, 6, 64])
@pytest.mark.parametrize("bits,ch,ms,trials", [(4, 2, False, 0), (4, 2, True, 2), (3, 1, False, 2), (2, 8, False, 0)])
def test_small_waves_and_chunks(engine, tile_kbytes, bits, ch, ms, trials):
    """a forced tile size: staging chunks of max(tile, 4 KiB) that cut through chains' PCM rows and output bytes, and device waves
    of 64 tiles that end between chains of one stream - a long stream mixed with many short ones spreads its chains over several
    waves, and at L = 64 a chain larger than a 64 KiB wave is a wave of its own - the bytes do not move"""
    spb = spb_of(ch, bits)
    rng = np.random.default_rng(tile_kbytes + bits + ch)
    lens = [int(v) for v in rng.integers(1, 3 * spb, 30)] + [(90 if ch < 8 else 30) * spb + 7] + [int(v) for v in rng.integers(1, spb, 20)]
    pcms = [synth_pcm(1, n, ch, seed=n + k)[0] for k, n in enumerate(lens)]
    param = make_parameter(ch, bits, MBS, 48000, ms, trials)
    engine.set_tile_kbytes(tile_kbytes)
    try:
        for L, W in ((4, 2), (16, 3), (1, 1), (64, 8)):
            got = engine.encode_host(pcms, param, segment_blocks=L, warmup_blocks=W)
            assert got == want_images(pcms, bits, L, W, ms=ms, trials=trials), (tile_kbytes, L, W)
            assert got == plan_images(engine, param, pcms, L, W), (tile_kbytes, L, W)
    finally:
        engine.set_tile_kbytes(0)


def test_long_stream_at_the_default_budget(engine):
    """stereo 4-bit at the CLI's block size, one stream past the 16 MiB staging chunk: one wave, several chunks each way"""
    pcm = synth_pcm(1, 4200 * spb_of(2, 4, 1024) + 333, 2, seed=77)[0]
    short = synth_pcm(1, 1000, 2, seed=78)[0]
    param = make_parameter(2, 4, 1024, 48000, False, 2)
    got = engine.encode_host([pcm, short], param, segment_blocks=64, warmup_blocks=8)
    assert got[0] == so.segmented_encode(pcm, 4, 64, 8, 1024, trials=2)
    assert got[1] == ob.encode(short, 4, 1024, 48000, False, 2)
    assert got == plan_images(engine, param, [pcm, short], 64, 8)


def test_encode_batch_refusals(engine):
    lib, ctx = engine.lib, engine._ctx
    param = make_parameter(2, 4, MBS, 48000, False, 2)
    x = np.zeros((1000, 2), dtype=np.int16)
    size = engine.encoded_size(param, 1000)
    out = np.zeros(size + 8, dtype=np.uint8)
    n = (C.c_uint32 * 1)(1000)
    pp, op = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
    cap, got = (C.c_uint64 * 1)(size), (C.c_uint64 * 1)(0)
    seg = AADHipSegmentation(4, 1)

    def call(c=ctx, p=param, s=seg, count=1, pcm=pp, ns=n, data=op, caps=cap):
        return lib.AADHip_SegmentedEncodeBatch(c, C.byref(p) if p is not None else None, C.byref(s) if s is not None else None,
                                               count, pcm, ns, data, caps, got)
    assert call() == AADApiResult.OK and got[0] == size
    assert call(c=None) == AADApiResult.INVALID_ARGUMENT
    assert call(p=None) == AADApiResult.INVALID_ARGUMENT
    assert call(s=None) == AADApiResult.INVALID_ARGUMENT
    assert call(s=AADHipSegmentation(0, 1)) == AADApiResult.INVALID_ARGUMENT
    assert call(pcm=None) == AADApiResult.INVALID_ARGUMENT
    assert call(pcm=(C.c_void_p * 1)(None)) == AADApiResult.INVALID_ARGUMENT
    assert call(data=(C.c_void_p * 1)(None)) == AADApiResult.INVALID_ARGUMENT
    assert call(caps=(C.c_uint64 * 1)(size - 1)) == AADApiResult.INSUFFICIENT_BUFFER
    assert call(ns=(C.c_uint32 * 1)(0)) == AADApiResult.INVALID_FORMAT
    assert call(p=make_parameter(2, 5, MBS, 48000, False, 0)) == AADApiResult.INVALID_FORMAT
    assert call(p=make_parameter(1, 4, MBS, 48000, True, 0)) == AADApiResult.INVALID_FORMAT
    assert call(count=0, pcm=None, ns=None, data=None, caps=None) == AADApiResult.OK
    # each the same code as AADHip_EncodeBatch where that has the case
    assert lib.AADHip_EncodeBatch(ctx, C.byref(param), 1, pp, n, op, (C.c_uint64 * 1)(size - 1), got, None) == AADApiResult.INSUFFICIENT_BUFFER
    assert lib.AADHip_EncodeBatch(ctx, C.byref(param), 1, pp, (C.c_uint32 * 1)(0), op, cap, got, None) == AADApiResult.INVALID_FORMAT


def _as_tuple(rec):
    return float(rec["rms_error"]), float(rec["mean_abs_error"]), float(rec["max_abs_error"])


@pytest.mark.parametrize("tile_kbytes", [0, 2])
@pytest.mark.parametrize("bits,ch,ms,trials", [(4, 2, False, 2), (3, 2, True, 0), (2, 1, False, 1), (4, 8, False, 0)])
def test_reconstruct_batch(engine, tile_kbytes, bits, ch, ms, trials):
    """AADHip_SegmentedReconstructBatch, in forced small chunks and waves too: the decoded output is the oracle's decode of the
    definition's image, the residual aado_residual's, the statistics aado_error_stats' bit for bit under the sequential order and
    the printed line the oracle's under the default order"""
    spb = spb_of(ch, bits, 1024)
    lens = [1, 5, spb, 3 * spb + 1, (40 if ch < 8 else 12) * spb - 9, 700]
    pcms = [synth_pcm(1, n, ch, seed=40 + n)[0] for n in lens]
    param = make_parameter(ch, bits, 1024, 48000, ms, trials)
    engine.set_tile_kbytes(tile_kbytes)
    try:
        for L, W in ((2, 1), (5, 0), (3, 7)):
            decoded = [ob.decode(img)[0] for img in want_images(pcms, bits, L, W, 1024, ms=ms, trials=trials)]
            engine.set_compare_order(sequential=True)
            rec, stats = engine.reconstruct_host(pcms, param, segment_blocks=L, warmup_blocks=W)
            gap, stats_g = engine.reconstruct_host(pcms, param, residual=True, segment_blocks=L, warmup_blocks=W)
            engine.set_compare_order(sequential=False)
            _, stats_d = engine.reconstruct_host(pcms, param, want_pcm=False, segment_blocks=L, warmup_blocks=W)
            for i, x in enumerate(pcms):
                where = (tile_kbytes, L, W, i, lens[i])
                assert np.array_equal(rec[i], decoded[i]), where
                assert np.array_equal(gap[i], ob.residual(x, decoded[i])), where
                want = ob.error_stats(x, decoded[i])
                assert _as_tuple(stats[i]) == want and _as_tuple(stats_g[i]) == want, where
                assert ob.stats_line(_as_tuple(stats_d[i])) == ob.stats_line(want), where
    finally:
        engine.set_compare_order(sequential=False)
        engine.set_tile_kbytes(0)


@pytest.mark.parametrize("residual", [False, True])
def test_reconstruct_plan(engine, residual):
    """AADHip_SegmentedReconstructPlanCreate + AADHip_ReconstructPlanRun (Engine.reconstruct_uniform)"""
    import torch
    bits, ch = 4, 2
    spb = spb_of(ch, bits, 1024)
    pcm = synth_pcm(6, 23 * spb - 17, ch, seed=5)
    param = make_parameter(ch, bits, 1024, 48000, False, 2)
    engine.set_compare_order(sequential=True)
    try:
        out, stats = engine.reconstruct_uniform(torch.from_numpy(pcm).cuda(), param, residual=residual, segment_blocks=4,
                                                warmup_blocks=2)
        torch.cuda.synchronize()
    finally:
        engine.set_compare_order(sequential=False)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    for s in range(pcm.shape[0]):
        y = ob.decode(so.segmented_encode(pcm[s], bits, 4, 2, 1024, trials=2))[0]
        assert np.array_equal(out[s], ob.residual(pcm[s], y) if residual else y), s
        assert tuple(float(v) for v in stats[s]) == ob.error_stats(pcm[s], y), s
    # the plain plan is untouched: the reference's images
    out0, _ = engine.reconstruct_uniform(torch.from_numpy(pcm).cuda(), param, residual=residual)
    torch.cuda.synchronize()
    y0 = ob.decode(ob.encode(pcm[0], bits, 1024, 48000, False, 2))[0]
    assert np.array_equal(out0.cpu().numpy()[0], ob.residual(pcm[0], y0) if residual else y0)


def test_reconstruct_refusals(engine):
    lib, ctx = engine.lib, engine._ctx
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    x = np.zeros((10, 2), dtype=np.int16)
    n = (C.c_uint32 * 1)(10)
    pp = (C.c_void_p * 1)(x.ctypes.data)
    seg = AADHipSegmentation(2, 1)
    assert lib.AADHip_SegmentedReconstructBatch(ctx, C.byref(param), None, 1, pp, n, 0, None, None) == AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_SegmentedReconstructBatch(ctx, C.byref(param), C.byref(AADHipSegmentation(0, 0)), 1, pp, n, 0, None,
                                                None) == AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_SegmentedReconstructBatch(None, C.byref(param), C.byref(seg), 1, pp, n, 0, None, None) == AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_SegmentedReconstructBatch(ctx, C.byref(param), C.byref(seg), 1, None, n, 0, None, None) == AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_SegmentedReconstructBatch(ctx, C.byref(param), C.byref(seg), 1, pp, n, 7, pp, None) == AADApiResult.INVALID_ARGUMENT
    bad = make_parameter(2, 5, 1024, 48000, False, 0)
    assert lib.AADHip_SegmentedReconstructBatch(ctx, C.byref(bad), C.byref(seg), 1, pp, n, 0, None, None) == AADApiResult.INVALID_FORMAT
    assert lib.AADHip_SegmentedReconstructBatch(ctx, C.byref(param), C.byref(seg), 0, None, None, 0, None, None) == AADApiResult.OK
    d = np.zeros(1, dtype=STREAM_DESC_DTYPE)
    d[0] = (0, 0, engine.encoded_size(param, 10), 10, 0)
    h = C.c_void_p()
    for s in (None, AADHipSegmentation(0, 3)):
        rc = lib.AADHip_SegmentedReconstructPlanCreate(ctx, C.byref(param), C.byref(s) if s is not None else None, 1, d.ctypes.data,
                                                       C.byref(h))
        assert rc == AADApiResult.INVALID_ARGUMENT and not h.value
    short = d.copy()
    short["data_size"][0] -= 1
    rc = lib.AADHip_SegmentedReconstructPlanCreate(ctx, C.byref(param), C.byref(seg), 1, short.ctypes.data, C.byref(h))
    assert rc == AADApiResult.INSUFFICIENT_BUFFER and not h.value
    rc = lib.AADHip_SegmentedReconstructPlanCreate(ctx, C.byref(param), C.byref(seg), 1, d.ctypes.data, C.byref(h))
    assert rc == AADApiResult.OK and h.value
    lib.AADHip_ReconstructPlanDestroy(h)


def test_python_surfaces(engine):
    bits, ch = 4, 2
    spb = spb_of(ch, bits, 1024)
    pcms = [synth_pcm(1, n, ch, seed=n)[0] for n in (9 * spb + 5, 100)]
    param = make_parameter(ch, bits, 1024)
    state = np.zeros(len(pcms) * ch, dtype=[("w", "<i4", 10)])
    with pytest.raises(ValueError):
        engine.encode_host(pcms, param, state=state, segment_blocks=2)
    with pytest.raises(ApiError) as e:
        engine.encode_host(pcms, param, segment_blocks=0)
    assert e.value.code == AADApiResult.INVALID_ARGUMENT
    with pytest.raises(ApiError) as e:
        engine.reconstruct_host(pcms, param, segment_blocks=0)
    assert e.value.code == AADApiResult.INVALID_ARGUMENT
    assert engine.encode_host(pcms, param, segment_blocks=2, warmup_blocks=1) == want_images(pcms, bits, 2, 1, 1024)
    assert engine.encode_host(pcms, param) == [ob.encode(p, bits, 1024) for p in pcms]  # the plain path is untouched
    rec, stats = engine.reconstruct_host(pcms, param, segment_blocks=3)
    assert np.array_equal(rec[0], ob.decode(so.segmented_encode(pcms[0], bits, 3, 0, 1024))[0])
    assert np.array_equal(rec[1], ob.decode(ob.encode(pcms[1], bits, 1024))[0])


@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_aad_batch_segment_blocks(tmp_path, devices):
    """aad_batch -e / -r / -g / -c -S on one long and one short WAV (CLI defaults: 4 bits, 1024-byte blocks, two trials): the long
    file gets the definition's image, the short one (at most L blocks: one chain) the reference's bytes"""
    assert os.path.exists(CLI), "aad_batch not built"
    ch, L, W = 2, 16, 3
    spb = spb_of(ch, 4, 1024)
    pcms = {"long": synth_pcm(1, 70 * spb + 123, ch, seed=11)[0], "short": synth_pcm(1, L * spb - 1, ch, seed=12)[0]}
    paths = []
    for name, pcm in pcms.items():
        p = tmp_path / (name + ".wav")
        p.write_bytes(wav16_bytes(pcm, 48000))
        paths.append(str(p))
    images = {n: so.segmented_encode(p, 4, L, W, 1024, trials=2) for n, p in pcms.items()}
    assert images["short"] == ob.encode(pcms["short"], 4, 1024, 48000, False, 2)
    assert images["long"] != ob.encode(pcms["long"], 4, 1024, 48000, False, 2)
    decoded = {n: ob.decode(images[n])[0] for n in pcms}
    opts = ["-S", "%d,%d" % (L, W), "-D", devices]
    for mode in ("-e", "-r", "-g"):
        out = tmp_path / (mode[1] + devices.replace(",", "_"))
        out.mkdir()
        subprocess.run([CLI, mode] + opts + ["-o", str(out)] + paths, check=True, timeout=300)
        for n, pcm in pcms.items():
            if mode == "-e":
                assert (out / (n + ".aad")).read_bytes() == images[n], (mode, n)
            else:
                got, rate = read_wav16(str(out / (n + ".wav")))
                assert rate == 48000
                assert np.array_equal(got, decoded[n] if mode == "-r" else ob.residual(pcm, decoded[n])), (mode, n)
    r = subprocess.run([CLI, "-c", "--segment-blocks", "%d,%d" % (L, W), "-D", devices] + paths, check=True, timeout=300,
                       capture_output=True, text=True)
    assert r.stdout == "".join("%s\t%s" % (p, ob.stats_line(ob.error_stats(pcms[n], decoded[n]))) for p, n in zip(paths, pcms))
    # without a warm-up: -S L means W = 0
    out = tmp_path / ("w0" + devices.replace(",", "_"))
    out.mkdir()
    subprocess.run([CLI, "-e", "-S", str(L), "-D", devices, "-o", str(out)] + paths, check=True, timeout=300)
    assert (out / "long.aad").read_bytes() == so.segmented_encode(pcms["long"], 4, L, 0, 1024, trials=2)
