"""Planar encode on the device (AADHip_PlanarEncodePlanCreate / AADHip_PlanarEncodePlanRun, Engine.encode_planar): int16 or
float32 rows per channel straight into .aad images.

Bar (include/aad_hip.h "planar encode"): the image bytes equal AADHip_EncodePlanRun's on the interleaved int16 P[t * C + c] =
q(x[c, t]) for the same parameter, table, segmentation and state - and, for a subset, the pinned oracle's
(tests/oracle_binding.encode, tests/segment_oracle.segmented_encode) directly.  Covered: channels 1, 2, 3 and 8; bits 2, 3 and
4; M/S on and off; trials 0, 1, 2 and 5; both sample types; every encode mapping forced, trial lanes dual and single, batch sizes
on both sides of the quad / dense and dual-layout switches; lengths of 1-4 frames, below one block, one block, one block + 1 and
many blocks, mixed in one plan; odd pcm_offsets and channel_stride > T; state carried across two runs; segmented (L, W) of
(1, 0), (3, 1) and (16, 4); canary bytes around every image and the input unchanged; float32 rows more than 4 GiB apart; the
float32 conversion observed exactly through the verbatim header samples of 4-frame streams; the API's errors, cross-use of the
two run functions, AADHip_ContextSignalNextRun events, ordering on a non-default torch stream, views."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import AADApiResult, AADHipPlanarLayout, AADHipSegmentation, SAMPLE_FLOAT32, SAMPLE_INT16, STREAM_DESC_DTYPE, make_parameter
from aad_amd.synth import synth_pcm

pytestmark = pytest.mark.gpu

CANARY = 0xA5
F32_SPECIALS_BITS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFBFFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                     0x00000001, 0x807FFFFF, 0x3F800000, 0xBF800000, 0x3F7FFE00, 0xBF7FFE00, 0x7F7FFFFF, 0xFF7FFFFF]


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def q(x):
    """include/aad_hip.h's q as torch states it (CPU), -> int16 numpy"""
    import torch
    if x.dtype == np.int16:
        return x.copy()
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return torch.nan_to_num(t, nan=0.0).mul(32768).round().clamp(-32768, 32767).to(torch.int16).numpy()


def make_rows(rng, channels, lengths, dtype, seed=1):
    """per stream a [C, n] array of the sample type: music-like int16, or for float32 the same / 32768 plus sub-LSB noise, exact
    ties and values past full scale, with the special bit patterns sprinkled in"""
    rows = []
    src = synth_pcm(len(lengths), max(lengths), channels, seed=seed)
    for i, n in enumerate(lengths):
        pcm = src[i, :n].T.copy()  # [C, n] int16
        if dtype == np.int16:
            rows.append(pcm)
            continue
        x = pcm.astype(np.float32) / 32768
        x += rng.uniform(-1.5, 1.5, size=x.shape).astype(np.float32) / 32768
        k = rng.random(x.shape)
        x[k < 0.05] = (np.round(x[k < 0.05] * 32768) + 0.5) / 32768      # exact ties
        x[(k >= 0.05) & (k < 0.07)] *= 3                                    # past full scale
        flat = x.reshape(-1)
        if flat.size >= 8:
            at = rng.choice(flat.size, size=min(len(F32_SPECIALS_BITS), flat.size // 4), replace=False)
            flat[at] = np.array(F32_SPECIALS_BITS[:len(at)], dtype=np.uint32).view(np.float32)
        rows.append(x.astype(np.float32))
    return rows


def lay_out(rows, channels, dtype, stride_pad=3, phase=3):
    """rows -> (flat buffer of the sample type, pcm_offsets, channel_stride): odd offsets, garbage between and around the rows"""
    cs = max(r.shape[1] for r in rows) + stride_pad
    offs, pos = [], phase
    for r in rows:
        offs.append(pos)
        pos += (channels - 1) * cs + r.shape[1] + 5
    rng = np.random.default_rng(99)
    if dtype == np.int16:
        buf = rng.integers(-32768, 32768, size=pos + 11).astype(np.int16)
    else:
        buf = rng.uniform(-4, 4, size=pos + 11).astype(np.float32)
        buf[::7] = np.nan
    for r, o in zip(rows, offs):
        for c in range(channels):
            buf[o + c * cs:o + c * cs + r.shape[1]] = r[c]
    return buf, np.array(offs, dtype=np.uint64), cs


def image_table(engine, param, lengths, gap=24, aligned=False):
    """images one after the other with canary gaps between and around them, every data_size exact; aligned: on 64-byte
    boundaries (the dense encoders' byte ring then serves the plan)"""
    t = np.zeros(len(lengths), dtype=STREAM_DESC_DTYPE)
    pos = gap
    for i, n in enumerate(lengths):
        pos = -(-pos // 64) * 64 if aligned else pos
        size = engine.encoded_size(param, int(n))
        t["data_offset"][i], t["data_size"][i], t["num_samples"][i] = pos, size, n
        pos += size + gap + (i % 3) * 7
    return t, pos + gap


def interleaved_run(engine, param, rows, table, total, seg=None, state=None):
    """AADHip_EncodePlanRun on P = q(rows) interleaved -> data buffer (numpy), state after"""
    import torch
    ch = rows[0].shape[0]
    parts, offs, pos = [], [], 0
    for r in rows:
        p = q(r).T.reshape(-1)
        offs.append(pos)
        parts.append(p)
        pos += p.size + 8
        parts.append(np.zeros(8, dtype=np.int16))
    pcm = torch.from_numpy(np.concatenate(parts)).cuda()
    t = table.copy()
    t["pcm_offset"] = offs
    plan = engine.encode_plan(param, t, *(seg or (None, 0)))
    data = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    st = None if state is None else state.clone()
    plan.run(pcm, data, st)
    torch.cuda.synchronize()
    plan.close()
    assert ch == param.num_channels
    return data.cpu().numpy(), st


def planar_run(engine, param, buf, offs, cs, table, total, seg=None, state=None, check_input=True):
    import torch
    dt = torch.float32 if buf.dtype == np.float32 else torch.int16
    x = torch.from_numpy(buf).cuda()
    t = table.copy()
    t["pcm_offset"] = offs
    plan = engine.planar_encode_plan(param, t, cs, dt, *(seg or (None, 0)))
    data = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    st = None if state is None else state.clone()
    plan.run(x, data, st)
    torch.cuda.synchronize()
    plan.close()
    if check_input:
        assert np.array_equal(x.cpu().numpy().view(np.uint8), buf.view(np.uint8)), "the input buffer changed"
    return data.cpu().numpy(), st


def check_canaries(data, table):
    mask = np.ones(data.size, dtype=bool)
    for d in table:
        mask[int(d["data_offset"]):int(d["data_offset"]) + int(d["data_size"])] = False
    assert (data[mask] == CANARY).all(), "a byte outside the images was written"


def compare(engine, param, rows, dtype, seg=None, oracle=False, trials=0, ms=False, aligned=False):
    buf, offs, cs = lay_out(rows, param.num_channels, dtype)
    lengths = [r.shape[1] for r in rows]
    table, total = image_table(engine, param, lengths, aligned=aligned)
    got, _ = planar_run(engine, param, buf, offs, cs, table, total, seg)
    want, _ = interleaved_run(engine, param, rows, table, total, seg)
    check_canaries(got, table)
    for i, d in enumerate(table):
        o, n = int(d["data_offset"]), int(d["data_size"])
        assert bytes(got[o:o + n]) == bytes(want[o:o + n]), "stream %d (%d frames) differs from the interleaved encode" % (i, lengths[i])
    assert np.array_equal(got, want)
    if oracle:
        for i, d in enumerate(table):
            o, n = int(d["data_offset"]), int(d["data_size"])
            p = q(rows[i]).T
            if seg is None:
                ref = ob.encode(p, param.bits_per_sample, 1024, 48000, ms, trials)
            else:
                ref = so.segmented_encode(p, param.bits_per_sample, seg[0], seg[1], ms=ms, trials=trials)
            assert bytes(got[o:o + n]) == ref, "stream %d differs from the oracle" % i


def lengths_for(spb):
    return [1, 2, 3, 4, spb // 2 + 3, spb, spb + 1, 5 * spb + 77, 4, spb - 1]


CASES = [(ch, bits, ms) for ch in (1, 2, 3, 8) for bits in (2, 3, 4) for ms in ((False, True) if ch == 2 else (False,))]


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("ch,bits,ms", CASES)
def test_matches_interleaved_and_oracle(engine, ch, bits, ms, dtype):
    trials = [0, 1, 2, 5][(ch + bits + ms) % 4]
    param = make_parameter(ch, bits, 1024, 48000, ms, trials)
    _, _, spb = ob.geometry(1024, ch, bits)
    rng = np.random.default_rng(ch * 100 + bits * 10 + ms)
    rows = make_rows(rng, ch, lengths_for(spb), dtype, seed=ch * 7 + bits)
    compare(engine, param, rows, dtype, oracle=True, trials=trials, ms=ms)


@pytest.mark.parametrize("mapping", ["auto", "dense", "quad", "quad-fused"])
@pytest.mark.parametrize("trial_lanes", ["dual", "single"])
def test_every_mapping(engine, mapping, trial_lanes):
    try:
        engine.set_mapping(mapping, trial_lanes)
        rng = np.random.default_rng(5)
        for ch, ms in ((1, False), (2, False), (2, True)):
            for bits in (4, 2):
                for trials in (0, 2):
                    # 40 streams: quad (and dual) territory under auto; 200: dense, and the single trial layout past the dual limit
                    for streams in (40, 200 if trials == 0 else 3000):
                        param = make_parameter(ch, bits, 1024, 48000, ms, trials)
                        _, _, spb = ob.geometry(1024, ch, bits)
                        lengths = [(spb + 1, 2 * spb, 3, spb - 5)[i % 4] for i in range(streams)]
                        rows = make_rows(rng, ch, lengths, np.float32 if streams % 3 else np.int16, seed=streams + bits)
                        compare(engine, param, rows, rows[0].dtype.type, ms=ms, trials=trials, aligned=streams == 200)
    finally:
        engine.set_mapping("auto", "dual")


@pytest.mark.parametrize("L,W", [(1, 0), (3, 1), (16, 4)])
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
def test_segmented(engine, L, W, dtype):
    rng = np.random.default_rng(L * 10 + W)
    for ch, bits, ms, trials in ((2, 4, False, 0), (2, 3, True, 2), (1, 2, False, 1), (3, 4, False, 0)):
        param = make_parameter(ch, bits, 1024, 48000, ms, trials)
        _, _, spb = ob.geometry(1024, ch, bits)
        lengths = [40 * spb + 13, 3, spb, 17 * spb, 2 * spb + 1]
        rows = make_rows(rng, ch, lengths, dtype, seed=bits + L)
        compare(engine, param, rows, dtype, seg=(L, W), oracle=ch <= 2, trials=trials, ms=ms)


def test_state_carried_across_two_runs(engine):
    import torch
    rng = np.random.default_rng(3)
    for ch, ms, dtype in ((2, True, np.float32), (2, False, np.int16), (3, False, np.float32), (1, False, np.float32)):
        param = make_parameter(ch, 4, 1024, 48000, ms, 2)
        _, _, spb = ob.geometry(1024, ch, 4)
        lengths = [spb + 9, 3 * spb, 2, 700]
        st_p = torch.zeros((len(lengths) * ch, 10), dtype=torch.int32, device="cuda")
        st_i = st_p.clone()
        for run in range(2):
            rows = make_rows(rng, ch, lengths, dtype, seed=run * 31 + ch)
            buf, offs, cs = lay_out(rows, ch, dtype)
            table, total = image_table(engine, param, lengths)
            got, st_p = planar_run(engine, param, buf, offs, cs, table, total, state=st_p)
            want, st_i = interleaved_run(engine, param, rows, table, total, state=st_i)
            assert np.array_equal(got, want), "run %d, %d channels" % (run, ch)
            assert torch.equal(st_p, st_i), "state records after run %d, %d channels" % (run, ch)


def test_view_with_channel_stride_above_T_equals_contiguous_copy(engine):
    import torch
    for dtype, ch, ms in ((torch.float32, 2, True), (torch.int16, 2, False), (torch.float32, 3, False), (torch.int16, 8, False)):
        param = make_parameter(ch, 4, 1024, 48000, ms, 1)
        big = torch.randn((7, ch + 1, 5000), device="cuda") * 0.3
        if dtype == torch.int16:
            big = (big * 32768).clamp(-32768, 32767).to(torch.int16)
        x = big[1:6, 1:, 3:3 + 2777]  # stride(1) = 5000 > T, odd element offset
        assert x.stride(-1) == 1 and not x.is_contiguous()
        lengths = [2777, 1, 1500, 4, 2048]
        a, sa = engine.encode_planar(x, param, num_samples=lengths)
        b, sb = engine.encode_planar(x.contiguous(), param, num_samples=lengths)
        assert sa == sb and torch.equal(a, b)
        xi = x.contiguous().cpu().numpy()
        for i, n in enumerate(lengths):
            assert bytes(a[i, :sa[i]].cpu().numpy()) == ob.encode(q(xi[i, :, :n]).T, 4, 1024, 48000, ms, 1), "row %d" % i
    with pytest.raises(ValueError, match="stride"):
        engine.encode_planar(torch.zeros((2, 2, 200), device="cuda")[:, :, ::2], make_parameter(2, 4))


def test_float32_conversion_exact_through_header_samples(engine):
    """Every block header carries its first four samples per channel verbatim and they decode verbatim (no M/S), so decoding
    4-frame streams gives q(v) itself: specials, ties, bounds and ~2^22 random bit patterns."""
    import torch
    rng = np.random.default_rng(11)
    f = np.float32
    special = np.array([0.0, -0.0, 1.0, -1.0, 32767 / 32768, -32767 / 32768, 32766.5 / 32768, -32768.5 / 32768, 0.5 / 32768,
                        -0.5 / 32768, 1.5 / 32768, -1.5 / 32768, 1e30, -1e30, np.inf, -np.inf, 1e-40, -1e-40], dtype=f)
    ties = ((np.arange(-32770, 32770) + 0.5) / 32768).astype(f)
    bits = np.array(F32_SPECIALS_BITS, dtype=np.uint32).view(f)
    rnd = rng.integers(0, 1 << 32, size=1 << 22, dtype=np.uint64).astype(np.uint32).view(f)
    v = np.concatenate([special, ties, bits, rnd])
    v = np.concatenate([v, np.zeros((-v.size) % 8, dtype=f)])
    x = torch.from_numpy(v.reshape(-1, 2, 4)).cuda()  # stereo, L/R, 4 frames
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    images, sizes = engine.encode_planar(x, param)
    dec, _ = engine.decode_uniform(images, sizes[0])
    torch.cuda.synchronize()
    got = dec.cpu().numpy().transpose(0, 2, 1).reshape(-1)  # [N, 4, 2] -> [N, 2, 4] -> v's order
    want = q(v)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "bits 0x%08x: decoded %d, q %d" % (v[bad[0]:bad[0] + 1].view(np.uint32)[0], got[bad[0]], want[bad[0]])


def test_rows_more_than_4gib_apart(engine):
    import torch
    free, _ = torch.cuda.mem_get_info()
    cs = (1 << 30) + 77  # floats: channel 1's row starts 4 GiB + 308 bytes after channel 0's
    if free < cs * 4 * 2 + (8 << 30):
        pytest.skip("needs %.1f GiB of free device memory" % (cs * 8 / 2 ** 30 + 8))
    param = make_parameter(2, 4, 1024, 48000, True, 0)
    _, _, spb = ob.geometry(1024, 2, 4)
    rng = np.random.default_rng(8)
    rows = make_rows(rng, 2, [3 * spb + 5, spb], np.float32, seed=4)
    buf = torch.zeros(cs + 2 * spb * 4 + 64, dtype=torch.float32, device="cuda")
    offs = [5, 5 + 3 * spb + 11]
    for r, o in zip(rows, offs):
        buf[o:o + r.shape[1]] = torch.from_numpy(r[0]).cuda()
        buf[o + cs:o + cs + r.shape[1]] = torch.from_numpy(r[1]).cuda()
    table, total = image_table(engine, param, [r.shape[1] for r in rows])
    t = table.copy()
    t["pcm_offset"] = offs
    plan = engine.planar_encode_plan(param, t, cs, torch.float32)
    data = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    plan.run(buf, data)
    torch.cuda.synchronize()
    plan.close()
    del buf
    got = data.cpu().numpy()
    check_canaries(got, table)
    for i, d in enumerate(table):
        o, n = int(d["data_offset"]), int(d["data_size"])
        assert bytes(got[o:o + n]) == ob.encode(q(rows[i]).T, 4, 1024, 48000, True, 0), "stream %d" % i


def _create(engine, param, layout, seg, table):
    plan = C.c_void_p()
    rc = engine.lib.AADHip_PlanarEncodePlanCreate(engine._ctx, C.byref(param), C.byref(layout) if layout is not None else None,
                                                  C.byref(seg) if seg is not None else None, len(table), table.ctypes.data,
                                                  C.byref(plan))
    return rc, plan


def test_api_errors_and_cross_use(engine):
    import torch
    param = make_parameter(2, 4)
    table, total = image_table(engine, param, [100, 50])
    table["pcm_offset"] = [0, 300]
    ok = AADHipPlanarLayout(SAMPLE_FLOAT32, 0, 100)
    IA = AADApiResult.INVALID_ARGUMENT
    assert _create(engine, param, None, None, table)[0] == IA
    assert _create(engine, param, AADHipPlanarLayout(2, 0, 100), None, table)[0] == IA
    assert _create(engine, param, AADHipPlanarLayout(-1, 0, 100), None, table)[0] == IA
    assert _create(engine, param, AADHipPlanarLayout(SAMPLE_INT16, 1, 100), None, table)[0] == IA
    assert _create(engine, param, AADHipPlanarLayout(SAMPLE_INT16, 0, 99), None, table)[0] == IA  # stride < num_samples
    assert _create(engine, param, ok, AADHipSegmentation(0, 0), table)[0] == IA
    big = table.copy()
    big["pcm_offset"][1] = (1 << 64) - 150  # element offset overflows
    assert _create(engine, param, ok, None, big)[0] == IA
    big["pcm_offset"][1] = (1 << 62) + 1000  # the element offset fits, the float32 byte offset does not
    assert _create(engine, param, ok, None, big)[0] == IA
    assert _create(engine, param, AADHipPlanarLayout(SAMPLE_FLOAT32, 0, (1 << 63)), None, table)[0] == IA  # (C-1) stride + n past 2^64 bytes
    rc, mono = _create(engine, make_parameter(1, 4), AADHipPlanarLayout(SAMPLE_INT16, 0, 0), None, table)  # mono: stride unused
    assert rc == AADApiResult.OK
    engine.lib.AADHip_EncodePlanDestroy(mono)
    short = table.copy()
    short["data_size"][0] -= 1
    assert _create(engine, param, ok, None, short)[0] == AADApiResult.INSUFFICIENT_BUFFER
    assert _create(engine, make_parameter(2, 1), ok, None, table)[0] == AADApiResult.INVALID_FORMAT

    x = torch.zeros(1000, dtype=torch.float32, device="cuda")
    data = torch.zeros(total, dtype=torch.uint8, device="cuda")
    state = torch.zeros((4, 10), dtype=torch.int32, device="cuda")
    rc, planar = _create(engine, param, ok, None, table)
    assert rc == AADApiResult.OK
    lib = engine.lib
    assert lib.AADHip_EncodePlanRun(planar, x.data_ptr(), data.data_ptr(), None) == IA      # planar plan, interleaved run
    assert lib.AADHip_PlanarEncodePlanRun(planar, None, data.data_ptr(), None) == IA
    assert lib.AADHip_PlanarEncodePlanRun(planar, x.data_ptr(), None, None) == IA
    assert lib.AADHip_PlanarEncodePlanRun(None, x.data_ptr(), data.data_ptr(), None) == IA
    assert lib.AADHip_PlanarEncodePlanRun(planar, x.data_ptr(), data.data_ptr(), state.data_ptr()) == AADApiResult.OK
    lib.AADHip_EncodePlanDestroy(planar)
    rc, seg = _create(engine, param, ok, AADHipSegmentation(1, 0), table)
    assert rc == AADApiResult.OK
    assert lib.AADHip_PlanarEncodePlanRun(seg, x.data_ptr(), data.data_ptr(), state.data_ptr()) == IA  # segmented: no state
    assert lib.AADHip_PlanarEncodePlanRun(seg, x.data_ptr(), data.data_ptr(), None) == AADApiResult.OK
    lib.AADHip_EncodePlanDestroy(seg)
    inter = engine.encode_plan(param, table)
    assert lib.AADHip_PlanarEncodePlanRun(inter.handle, x.data_ptr(), data.data_ptr(), None) == IA  # interleaved plan, planar run
    inter.close()
    empty = np.zeros(0, dtype=STREAM_DESC_DTYPE)
    rc, e = _create(engine, param, ok, None, empty)
    assert rc == AADApiResult.OK and lib.AADHip_PlanarEncodePlanRun(e, x.data_ptr(), data.data_ptr(), None) == AADApiResult.OK
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
        x = torch.randn((64, 2, 9000), device="cuda") * 0.4  # queued on `side`, not yet run when the encode is queued
        start, stop = HipEvent(timing=True), HipEvent(timing=True)
        eng.signal_next(stop, start=start)
        images, sizes = eng.encode_planar(x, param)
        stop.synchronize()
        assert start.elapsed_ms(stop) > 0
        ref, rs = engine.encode_planar(x.contiguous(), param)
    torch.cuda.synchronize()
    assert sizes == rs and torch.equal(images, ref)
    xi = x.cpu().numpy()
    assert bytes(images[5, :sizes[5]].cpu().numpy()) == ob.encode(q(xi[5]).T, 4, 1024)
    start.close()
    stop.close()
    eng.close()
