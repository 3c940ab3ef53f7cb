"""Planar reconstruct on the device (AADHip_PlanarReconstructPlanCreate / AADHip_PlanarReconstructPlanRun,
Engine.reconstruct_planar): [N, C, T] int16 / float32 rows through the codec in one kernel.

Bar (include/aad_hip.h "planar reconstruct"): the images are byte-equal to the planar encode's (AADHip_PlanarEncodePlanRun) for the
same plan inputs, and every output row equals AADHip_DecodePlanRun of its image, converted (int16, or / 32768 bit for bit as
float32); on a subset the decode is also the pinned oracle's (tests/oracle_binding.decode).  Covered: channels 1, 2, 3, 8; bits
2, 3, 4; M/S on and off; trials 0, 1, 2, 5; all four sample-type pairs; every mapping forced with trial lanes dual and single;
batch sizes on both sides of the quad / dense switch; lengths 1-5, spb - 1, spb, spb + 1 and many blocks mixed in one plan; odd
offsets, channel strides above T and output strides unlike the input's; state across two runs; segmented (1, 0), (3, 1), (16, 4);
canaries around every output row and image with the input unchanged; float32 specials through the verbatim header samples; output
rows more than 4 GiB apart; the API errors, cross-use refusals, the events on the one kernel and a non-default torch stream."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from aad_amd.capi import (AADApiResult, AADHipPlanarLayout, AADHipPlanarOutput, AADHipSegmentation, SAMPLE_FLOAT32, SAMPLE_INT16,
                          STREAM_DESC_DTYPE, make_parameter)
from test_gpu_planar_encode import CANARY, F32_SPECIALS_BITS, check_canaries, image_table, lay_out, make_rows, q

pytestmark = pytest.mark.gpu

OUT_CANARY_I16 = 0x5A5A
OUT_CANARY_F32 = 0x7FA5A5A5  # a NaN no conversion produces


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def tdt(dtype):
    import torch
    return torch.float32 if dtype == np.float32 else torch.int16


def out_buffer(n_elems, out_dtype):
    import torch
    if out_dtype == np.float32:
        return torch.full((n_elems,), OUT_CANARY_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n_elems,), OUT_CANARY_I16, dtype=torch.int16, device="cuda")


def decode_images(engine, param, data, table):
    """AADHip_DecodePlanRun of every image of `data` (numpy bytes) -> list of [n, C] int16"""
    import torch
    from aad_amd.engine import parse_header
    lengths = [int(v) for v in table["num_samples"]]
    ch = param.num_channels
    head = parse_header(bytes(data[int(table["data_offset"][0]):int(table["data_offset"][0]) + 31]))
    d = table.copy()
    d["pcm_offset"] = np.concatenate([[0], np.cumsum(np.array(lengths, dtype=np.uint64) * ch)[:-1]]).astype(np.uint64)
    plan = engine.decode_plan(head, d, True)
    pcm = torch.zeros(sum(lengths) * ch + 1, dtype=torch.int16, device="cuda")
    plan.run(torch.from_numpy(data).cuda(), pcm)
    torch.cuda.synchronize()
    plan.close()
    flat = pcm.cpu().numpy()
    return [flat[int(o):int(o) + n * ch].reshape(n, ch) for o, n in zip(d["pcm_offset"], lengths)]


def run_case(engine, param, rows, in_dtype, out_dtype, seg=None, state=None, oracle=False, aligned=False, st_enc=None):
    """one reconstruct run against the planar encode and AADHip_DecodePlanRun; returns the state records after the run"""
    import torch
    ch = param.num_channels
    buf, offs, cs = lay_out(rows, ch, in_dtype)
    lengths = [r.shape[1] for r in rows]
    table, total = image_table(engine, param, lengths, aligned=aligned)
    table["pcm_offset"] = offs
    ocs = max(lengths) + 5                   # output rows: a gap behind each channel's row
    oss = ch * ocs + 13                      # and behind each stream
    base = 7
    n_out = base + len(rows) * oss + 11
    x = torch.from_numpy(buf).cuda()
    out_full = out_buffer(n_out, out_dtype)
    data = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    plan = engine.planar_reconstruct_plan(param, table, cs, tdt(in_dtype), tdt(out_dtype), oss, ocs, *(seg or (None, 0)))
    st = None if state is None else state.clone()
    plan.run(x, data, out_full[base:], st)
    torch.cuda.synchronize()
    plan.close()
    assert np.array_equal(x.cpu().numpy().view(np.uint8), buf.view(np.uint8)), "the input buffer changed"
    got = data.cpu().numpy()
    # the images: exactly the planar encode's
    enc = engine.planar_encode_plan(param, table, cs, tdt(in_dtype), *(seg or (None, 0)))
    want = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    st2 = None if st_enc is None else st_enc.clone()
    enc.run(x, want, st2)
    torch.cuda.synchronize()
    enc.close()
    check_canaries(got, table)
    assert np.array_equal(got, want.cpu().numpy()), "the images differ from the planar encode's"
    if st is not None:
        assert torch.equal(st, st2), "state records differ from the planar encode's"
    # the rows: the decode of those images, converted, canaries everywhere else
    dec = decode_images(engine, param, got, table)
    o = out_full.cpu().numpy()
    # compared as bit patterns: float32 output bit for bit, the canary NaN included
    ubits = np.uint32 if out_dtype == np.float32 else np.uint16
    expect = np.full(o.size, OUT_CANARY_F32 if out_dtype == np.float32 else OUT_CANARY_I16, dtype=ubits)
    for i, d in enumerate(dec):
        for c in range(ch):
            at = base + i * oss + c * ocs
            v = d[:, c].astype(np.float32) / np.float32(32768) if out_dtype == np.float32 else d[:, c].astype(np.int16)
            expect[at:at + d.shape[0]] = v.view(ubits)
    bad = np.flatnonzero(o.view(ubits) != expect)
    if bad.size:
        e = int(bad[0]) - base
        i, r = e // oss, e % oss
        pytest.fail("output element %d (stream %d of %d frames, channel %d, frame %d): got %r, want %r (%d bad)" % (
            bad[0], i, lengths[i] if i < len(lengths) else -1, r // ocs, r % ocs, o.view(ubits)[bad[0]], expect[bad[0]], bad.size))
    if oracle:
        for i, d in enumerate(table):
            img = bytes(got[int(d["data_offset"]):int(d["data_offset"]) + int(d["data_size"])])
            assert np.array_equal(ob.decode(img)[0], dec[i]), "stream %d: AADHip_DecodePlanRun differs from the oracle" % i
    return st


def lengths_for(spb):
    return [1, 2, 3, 4, 5, spb // 2 + 3, spb, spb + 1, 5 * spb + 77, spb - 1]


CASES = [(ch, bits, ms) for ch in (1, 2, 3, 8) for bits in (2, 3, 4) for ms in ((False, True) if ch == 2 else (False,))]
TYPES = [(np.int16, np.int16), (np.int16, np.float32), (np.float32, np.int16), (np.float32, np.float32)]


@pytest.mark.parametrize("types", TYPES, ids=["i16-i16", "i16-f32", "f32-i16", "f32-f32"])
@pytest.mark.parametrize("ch,bits,ms", CASES)
def test_matches_encode_and_decode(engine, ch, bits, ms, types):
    trials = [0, 1, 2, 5][(ch + bits + ms) % 4]
    param = make_parameter(ch, bits, 1024, 48000, ms, trials)
    _, _, spb = ob.geometry(1024, ch, bits)
    rng = np.random.default_rng(ch * 100 + bits * 10 + ms)
    rows = make_rows(rng, ch, lengths_for(spb), types[0], seed=ch * 7 + bits)
    run_case(engine, param, rows, types[0], types[1], oracle=types == (np.float32, np.float32) or ch == 2)


@pytest.mark.parametrize("mapping", ["auto", "dense", "quad", "quad-fused"])
@pytest.mark.parametrize("trial_lanes", ["dual", "single"])
def test_every_mapping(engine, mapping, trial_lanes):
    try:
        engine.set_mapping(mapping, trial_lanes)
        rng = np.random.default_rng(5)
        for ch, ms in ((1, False), (2, False), (2, True)):
            for bits in (4, 3, 2):
                for trials in (0, 2):
                    # 40 streams: quad territory under auto; 200 / 3000: dense, and past the dual search's limit
                    for streams in (40, 200 if trials == 0 else 3000):
                        param = make_parameter(ch, bits, 1024, 48000, ms, trials)
                        _, _, spb = ob.geometry(1024, ch, bits)
                        lengths = [(spb + 1, 2 * spb, 3, spb - 5)[i % 4] for i in range(streams)]
                        dt = np.float32 if streams % 3 else np.int16
                        rows = make_rows(rng, ch, lengths, dt, seed=streams + bits)
                        run_case(engine, param, rows, dt, np.float32 if bits != 3 else np.int16, aligned=streams == 200)
    finally:
        engine.set_mapping("auto", "dual")


@pytest.mark.parametrize("L,W", [(1, 0), (3, 1), (16, 4)])
@pytest.mark.parametrize("types", [(np.int16, np.float32), (np.float32, np.int16)], ids=["i16-f32", "f32-i16"])
def test_segmented(engine, L, W, types):
    rng = np.random.default_rng(L * 10 + W)
    for ch, bits, ms, trials in ((2, 4, False, 0), (2, 3, True, 2), (1, 2, False, 1), (3, 4, False, 0), (1, 4, False, 0)):
        param = make_parameter(ch, bits, 1024, 48000, ms, trials)
        _, _, spb = ob.geometry(1024, ch, bits)
        lengths = [40 * spb + 13, 3, spb, 17 * spb, 2 * spb + 1]
        rows = make_rows(rng, ch, lengths, types[0], seed=bits + L)
        run_case(engine, param, rows, types[0], types[1], seg=(L, W), oracle=ch <= 2)


def test_state_carried_across_two_runs(engine):
    import torch
    rng = np.random.default_rng(3)
    for ch, ms, dtype in ((2, True, np.float32), (2, False, np.int16), (3, False, np.float32), (1, False, np.int16)):
        param = make_parameter(ch, 4, 1024, 48000, ms, 2)
        _, _, spb = ob.geometry(1024, ch, 4)
        lengths = [spb + 9, 3 * spb, 2, 700]
        st = torch.zeros((len(lengths) * ch, 10), dtype=torch.int32, device="cuda")
        for run in range(2):
            rows = make_rows(rng, ch, lengths, dtype, seed=run * 31 + ch)
            st = run_case(engine, param, rows, dtype, np.float32, state=st, st_enc=st)


def test_reconstruct_planar_views_dtypes_and_images(engine):
    import torch
    for dtype, ch, ms in ((torch.float32, 2, True), (torch.int16, 2, False), (torch.float32, 3, False), (torch.int16, 1, False)):
        param = make_parameter(ch, 3, 1024, 48000, ms, 1)
        big = torch.randn((7, ch + 1, 5000), device="cuda") * 0.3
        if dtype == torch.int16:
            big = (big * 32768).clamp(-32768, 32767).to(torch.int16)
        x = big[1:6, 1:, 3:3 + 2777]  # stride(1) = 5000 > T, odd element offset
        assert x.stride(-1) == 1 and not x.is_contiguous()
        lengths = [2777, 1, 1500, 4, 2048]
        for out_dtype in (None, torch.int16, torch.float32):
            y, images, sizes = engine.reconstruct_planar(x, param, num_samples=lengths, dtype=out_dtype, return_images=True)
            assert y.dtype == (out_dtype or dtype) and y.shape == x.shape and y.is_contiguous()
            ref, rs = engine.encode_planar(x.contiguous(), param, num_samples=lengths)
            assert sizes == rs and torch.equal(images, ref)
            y2 = engine.reconstruct_planar(x.contiguous(), param, num_samples=lengths, dtype=out_dtype)
            assert torch.equal(y.view(torch.int16 if y.dtype == torch.int16 else torch.int32),
                               y2.view(torch.int16 if y2.dtype == torch.int16 else torch.int32))
            yc = y.cpu().numpy()
            for i, n in enumerate(lengths):
                dec = ob.decode(bytes(images[i, :sizes[i]].cpu().numpy()))[0]  # [n, C]
                want = dec.T.astype(np.float32) / np.float32(32768) if y.dtype == torch.float32 else dec.T
                assert np.array_equal(yc[i, :, :n], want), "row %d" % i
                assert not yc[i, :, n:].any(), "row %d: not zero past num_samples" % i
    with pytest.raises(ValueError, match="stride"):
        engine.reconstruct_planar(torch.zeros((2, 2, 200), device="cuda")[:, :, ::2], make_parameter(2, 4))


def test_float32_specials_through_header_samples(engine):
    """4-frame streams are header samples only: the output is q(v) itself (no M/S), or q(v) / 32768 as float32"""
    import torch
    rng = np.random.default_rng(11)
    f = np.float32
    special = np.array([0.0, -0.0, 1.0, -1.0, 32767 / 32768, -32767 / 32768, 32766.5 / 32768, -32768.5 / 32768, 0.5 / 32768,
                        -0.5 / 32768, 1e30, -1e30, np.inf, -np.inf, 1e-40, -1e-40], dtype=f)
    bits = np.array(F32_SPECIALS_BITS, dtype=np.uint32).view(f)
    rnd = rng.integers(0, 1 << 32, size=1 << 18, dtype=np.uint64).astype(np.uint32).view(f)
    v = np.concatenate([special, bits, rnd])
    v = np.concatenate([v, np.zeros((-v.size) % 8, dtype=f)])
    x = torch.from_numpy(v.reshape(-1, 2, 4)).cuda()
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    yi = engine.reconstruct_planar(x, param, dtype=torch.int16)
    yf = engine.reconstruct_planar(x, param, dtype=torch.float32)
    torch.cuda.synchronize()
    want = q(v)
    assert np.array_equal(yi.cpu().numpy().reshape(-1), want)
    assert np.array_equal(yf.cpu().numpy().reshape(-1).view(np.uint32), (want.astype(np.float32) / np.float32(32768)).view(np.uint32))


def test_output_rows_more_than_4gib_apart(engine):
    import torch
    free, _ = torch.cuda.mem_get_info()
    ocs = (1 << 30) + 77  # floats: channel 1's output row starts 4 GiB + 308 bytes after channel 0's
    if free < ocs * 4 * 3 + (8 << 30):
        pytest.skip("needs %.1f GiB of free device memory" % (ocs * 12 / 2 ** 30 + 8))
    param = make_parameter(2, 4, 1024, 48000, True, 0)
    _, _, spb = ob.geometry(1024, 2, 4)
    rng = np.random.default_rng(8)
    lengths = [3 * spb + 5, spb]
    rows = make_rows(rng, 2, lengths, np.float32, seed=4)
    buf, offs, cs = lay_out(rows, 2, np.float32)
    table, total = image_table(engine, param, lengths)
    table["pcm_offset"] = offs
    oss = ocs + 4 * spb  # stream 1's rows behind stream 0's channel-1 row: 8 GiB in
    out = torch.full((oss + ocs + 4 * spb,), -7.0, dtype=torch.float32, device="cuda")
    plan = engine.planar_reconstruct_plan(param, table, cs, torch.float32, torch.float32, oss, ocs)
    data = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    plan.run(torch.from_numpy(buf).cuda(), data, out)
    torch.cuda.synchronize()
    plan.close()
    got = data.cpu().numpy()
    check_canaries(got, table)
    for i, d in enumerate(table):
        img = bytes(got[int(d["data_offset"]):int(d["data_offset"]) + int(d["data_size"])])
        assert img == ob.encode(q(rows[i]).T, 4, 1024, 48000, True, 0), "stream %d" % i
        dec = ob.decode(img)[0]
        for c in range(2):
            at = i * oss + c * ocs
            row = out[at:at + lengths[i] + 3].cpu().numpy()
            assert np.array_equal(row[:lengths[i]], dec[:, c].astype(np.float32) / np.float32(32768)), "stream %d channel %d" % (i, c)
            assert (row[lengths[i]:] == -7.0).all()
    del out


def _create(engine, param, layout, output, seg, table):
    plan = C.c_void_p()
    rc = engine.lib.AADHip_PlanarReconstructPlanCreate(engine._ctx, C.byref(param), C.byref(layout) if layout is not None else None,
                                                       C.byref(output) if output is not None else None,
                                                       C.byref(seg) if seg is not None else None, len(table), table.ctypes.data,
                                                       C.byref(plan))
    return rc, plan


def test_api_errors_and_cross_use(engine):
    import torch
    param = make_parameter(2, 4)
    table, total = image_table(engine, param, [100, 50])
    table["pcm_offset"] = [0, 300]
    lay = AADHipPlanarLayout(SAMPLE_FLOAT32, 0, 100)
    out_ok = AADHipPlanarOutput(SAMPLE_FLOAT32, 0, 200, 100)
    IA = AADApiResult.INVALID_ARGUMENT
    assert _create(engine, param, lay, None, None, table)[0] == IA
    assert _create(engine, param, None, out_ok, None, table)[0] == IA
    assert _create(engine, param, AADHipPlanarLayout(SAMPLE_INT16, 0, 99), out_ok, None, table)[0] == IA  # the encode's errors
    assert _create(engine, param, lay, out_ok, AADHipSegmentation(0, 0), table)[0] == IA
    for bad in (AADHipPlanarOutput(2, 0, 200, 100), AADHipPlanarOutput(-1, 0, 200, 100), AADHipPlanarOutput(SAMPLE_INT16, 1, 200, 100),
                AADHipPlanarOutput(SAMPLE_INT16, 0, 200, 99),       # channel rows overlap
                AADHipPlanarOutput(SAMPLE_INT16, 0, 199, 100),      # stream rows overlap
                AADHipPlanarOutput(SAMPLE_INT16, 0, 1 << 63, 100),  # (N - 1) stream_stride + span: fits elements, not bytes
                AADHipPlanarOutput(SAMPLE_FLOAT32, 0, 1 << 62, 100)):
        assert _create(engine, param, lay, bad, None, table)[0] == IA
    short = table.copy()
    short["data_size"][0] -= 1
    assert _create(engine, param, lay, out_ok, None, short)[0] == AADApiResult.INSUFFICIENT_BUFFER
    assert _create(engine, make_parameter(2, 1), lay, out_ok, None, table)[0] == AADApiResult.INVALID_FORMAT

    x = torch.zeros(1000, dtype=torch.float32, device="cuda")
    data = torch.zeros(total, dtype=torch.uint8, device="cuda")
    out = torch.zeros(400, dtype=torch.float32, device="cuda")
    state = torch.zeros((4, 10), dtype=torch.int32, device="cuda")
    lib = engine.lib
    rc, rec = _create(engine, param, lay, out_ok, None, table)
    assert rc == AADApiResult.OK
    assert lib.AADHip_EncodePlanRun(rec, x.data_ptr(), data.data_ptr(), None) == IA            # a reconstruct plan, the other runs
    assert lib.AADHip_PlanarEncodePlanRun(rec, x.data_ptr(), data.data_ptr(), None) == IA
    assert lib.AADHip_PlanarReconstructPlanRun(rec, None, data.data_ptr(), out.data_ptr(), None) == IA
    assert lib.AADHip_PlanarReconstructPlanRun(rec, x.data_ptr(), None, out.data_ptr(), None) == IA
    assert lib.AADHip_PlanarReconstructPlanRun(rec, x.data_ptr(), data.data_ptr(), None, None) == IA
    assert lib.AADHip_PlanarReconstructPlanRun(rec, x.data_ptr(), data.data_ptr(), x.data_ptr(), None) == IA  # out == input
    assert lib.AADHip_PlanarReconstructPlanRun(None, x.data_ptr(), data.data_ptr(), out.data_ptr(), None) == IA
    assert lib.AADHip_PlanarReconstructPlanRun(rec, x.data_ptr(), data.data_ptr(), out.data_ptr(), state.data_ptr()) == AADApiResult.OK
    lib.AADHip_EncodePlanDestroy(rec)
    rc, seg = _create(engine, param, lay, out_ok, AADHipSegmentation(1, 0), table)
    assert rc == AADApiResult.OK
    assert lib.AADHip_PlanarReconstructPlanRun(seg, x.data_ptr(), data.data_ptr(), out.data_ptr(), state.data_ptr()) == IA
    assert lib.AADHip_PlanarReconstructPlanRun(seg, x.data_ptr(), data.data_ptr(), out.data_ptr(), None) == AADApiResult.OK
    lib.AADHip_EncodePlanDestroy(seg)
    planar = engine.planar_encode_plan(param, table, 100, torch.float32)
    assert lib.AADHip_PlanarReconstructPlanRun(planar.handle, x.data_ptr(), data.data_ptr(), out.data_ptr(), None) == IA
    planar.close()
    inter = engine.encode_plan(param, table)
    assert lib.AADHip_PlanarReconstructPlanRun(inter.handle, x.data_ptr(), data.data_ptr(), out.data_ptr(), None) == IA
    inter.close()
    empty = np.zeros(0, dtype=STREAM_DESC_DTYPE)
    rc, e = _create(engine, param, lay, out_ok, None, empty)
    assert rc == AADApiResult.OK and lib.AADHip_PlanarReconstructPlanRun(e, x.data_ptr(), data.data_ptr(), None, None) == AADApiResult.OK
    lib.AADHip_EncodePlanDestroy(e)
    torch.cuda.synchronize()


def test_signal_events_and_non_default_stream(engine):
    import torch
    from aad_amd.engine import Engine, HipEvent
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = Engine(0)
        assert eng.stream.cuda_stream == side.cuda_stream
        x = torch.randn((64, 2, 9000), device="cuda") * 0.4  # queued on `side`, not yet run when the reconstruct is queued
        start, stop = HipEvent(timing=True), HipEvent(timing=True)
        eng.signal_next(stop, start=start)
        y, images, sizes = eng.reconstruct_planar(x, param, return_images=True)
        stop.synchronize()
        assert start.elapsed_ms(stop) > 0
        ref, rs = engine.encode_planar(x.contiguous(), param)
    torch.cuda.synchronize()
    assert sizes == rs and torch.equal(images, ref)
    dec = ob.decode(bytes(images[5, :sizes[5]].cpu().numpy()))[0]
    assert np.array_equal(y[5].cpu().numpy(), dec.T.astype(np.float32) / np.float32(32768))
    start.close()
    stop.close()
    eng.close()
