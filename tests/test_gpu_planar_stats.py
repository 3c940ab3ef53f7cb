"""Planar reconstruct statistics on the device (AADHip_PlanarReconstructPlanRunStats, PlanarReconstructPlan.run(stats=...),
Engine.reconstruct_planar(return_stats=True), Engine.codec_error, Engine.least_bits).

Bar (include/aad_hip.h "planar reconstruct statistics"): == on every integer of every record, no tolerance.  Expected values:
e = q(x).astype(int64) - D with D the int16 rows a plain AADHip_PlanarReconstructPlanRun of the same plan inputs writes (pinned to
AADHip_DecodePlanRun and the oracle by tests/test_gpu_planar_reconstruct.py), summed in numpy int64; on a subset D also comes from
oracle_binding encode + decode directly.  Every case also demands: images, rows and state byte-equal to the run without
statistics, canaries around the table, the rows and the images, the input unchanged, and a second run into a table holding other
garbage giving the same records.

A stream of length 0 cannot be in a plan: the plan constructors refuse it (AAD_APIRESULT_INVALID_FORMAT, as the reference
encoder refuses an empty input) - test_api_errors_and_cross_use pins that; the empty row of the definition is covered by the CPU
tests of rmse / snr_db."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from aad_amd.capi import (AADApiResult, AADHipPlanarLayout, AADHipPlanarOutput, AADHipSegmentation, SAMPLE_FLOAT32,
                          STREAM_DESC_DTYPE, make_parameter)
from test_gpu_planar_encode import CANARY, F32_SPECIALS_BITS, check_canaries, image_table, lay_out, make_rows, q
from test_gpu_planar_reconstruct import out_buffer, tdt

pytestmark = pytest.mark.gpu

STATS_CANARY = -0x5A5A5A5A5A5A5A5B
PAD = 9  # int64 elements of canary in front of and behind the table


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def expected_stats(rows, dec):
    """rows: per stream [C, n] input; dec: per stream [C, n] int16 decoded -> int64 [N, C, 4]"""
    want = np.zeros((len(rows), rows[0].shape[0], 4), dtype=np.int64)
    for i, (r, d) in enumerate(zip(rows, dec)):
        e = q(r).astype(np.int64) - d.astype(np.int64)
        want[i, :, 0] = (e * e).sum(axis=1)
        want[i, :, 1] = np.abs(e).sum(axis=1)
        want[i, :, 2] = np.abs(e).max(axis=1) if e.shape[1] else 0
        want[i, :, 3] = e.shape[1]
    return want


def stats_table(n, ch, seed):
    """a garbage-filled [n, ch, 4] view inside a canary-padded int64 buffer"""
    import torch
    full = torch.full((2 * PAD + n * ch * 4,), STATS_CANARY, dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    full[PAD:PAD + n * ch * 4] = torch.randint(-2 ** 62, 2 ** 62, (n * ch * 4,), generator=g, device="cuda", dtype=torch.int64)
    return full, full[PAD:PAD + n * ch * 4].view(n, ch, 4)


def check_stats_canaries(full):
    f = full.cpu().numpy()
    assert (f[:PAD] == STATS_CANARY).all() and (f[-PAD:] == STATS_CANARY).all(), "an element outside the statistics table was written"


def run_stats_case(engine, param, rows, in_dtype, out_dtype, seg=None, state=None, oracle=False, aligned=False):
    """one statistics run (out_dtype None: device_out = NULL) against the plain reconstruct runs; returns (records, state after)"""
    import torch
    ch = param.num_channels
    n = len(rows)
    buf, offs, cs = lay_out(rows, ch, in_dtype)
    lengths = [r.shape[1] for r in rows]
    table, total = image_table(engine, param, lengths, aligned=aligned)
    table["pcm_offset"] = offs
    ocs = max(lengths) + 5
    oss = ch * ocs + 13
    base = 7
    n_out = base + n * oss + 11
    x = torch.from_numpy(buf).cuda()
    segargs = seg or (None, 0)

    def plain(dt):
        out = out_buffer(n_out, dt)
        data = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        plan = engine.planar_reconstruct_plan(param, table, cs, tdt(in_dtype), tdt(dt), oss, ocs, *segargs)
        st = None if state is None else state.clone()
        plan.run(x, data, out[base:], st)
        torch.cuda.synchronize()
        plan.close()
        return out, data, st

    ref16, ref_data, ref_st = plain(np.int16)
    ref_out = ref16 if out_dtype in (None, np.int16) else plain(out_dtype)[0]
    r16 = ref16.cpu().numpy()
    dec = [np.stack([r16[base + i * oss + c * ocs:base + i * oss + c * ocs + lengths[i]] for c in range(ch)]) for i in range(n)]
    want = expected_stats(rows, dec)

    plan = engine.planar_reconstruct_plan(param, table, cs, tdt(in_dtype), tdt(out_dtype or np.int16), oss, ocs, *segargs)
    got = []
    for attempt in range(2):
        full, stats = stats_table(n, ch, seed=attempt + 1)
        out = None if out_dtype is None else out_buffer(n_out, out_dtype)
        data = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        st = None if state is None else state.clone()
        plan.run(x, data, None if out is None else out[base:], st, stats=stats)
        torch.cuda.synchronize()
        check_stats_canaries(full)
        check_canaries(data.cpu().numpy(), table)
        assert torch.equal(data, ref_data), "the images differ from the run without statistics"
        if out is not None:
            bits = torch.int32 if out_dtype == np.float32 else torch.int16
            assert torch.equal(out.view(bits), ref_out.view(bits)), "the rows (or their canaries) differ from the run without statistics"
        if st is not None:
            assert torch.equal(st, ref_st), "the state records differ from the run without statistics"
        got.append(stats.cpu().numpy().copy())
    plan.close()
    assert np.array_equal(x.cpu().numpy().view(np.uint8), buf.view(np.uint8)), "the input buffer changed"
    assert np.array_equal(got[0], got[1]), "two runs gave different tables"
    bad = np.argwhere(got[0] != want)
    if bad.size:
        i, c, f = (int(v) for v in bad[0])
        pytest.fail("stream %d (%d frames) channel %d field %d: got %d, want %d (%d records differ)" % (
            i, lengths[i], c, f, got[0][i, c, f], want[i, c, f], len({(int(a), int(b)) for a, b, _ in bad})))
    if oracle:
        assert seg is None and state is None
        ms = param.ch_process_method != 0
        odec = []
        for r in rows:
            img = ob.encode(np.ascontiguousarray(q(r).T), param.bits_per_sample, param.max_block_size, param.sampling_rate, ms,
                            param.num_encode_trials)
            odec.append(ob.decode(img)[0].T)
        assert np.array_equal(got[0], expected_stats(rows, odec)), "the records differ from those of the oracle's encode + decode"
    return got[0], st


def lengths_for(spb):
    return [1, 2, 3, 4, 5, 15, 16, 17, spb // 2 + 3, spb, spb + 1, 5 * spb + 77, spb - 1]


CASES = [(ch, bits, ms) for ch in (1, 2, 3, 8) for bits in (2, 3, 4) for ms in ((False, True) if ch == 2 else (False,))]
TYPES = [(np.int16, np.int16), (np.int16, np.float32), (np.float32, np.int16), (np.float32, np.float32), (np.int16, None),
         (np.float32, None)]
TYPE_IDS = ["i16-i16", "i16-f32", "f32-i16", "f32-f32", "i16-none", "f32-none"]


@pytest.mark.parametrize("types", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("ch,bits,ms", CASES)
def test_records_exact(engine, ch, bits, ms, types):
    trials = (0, 2)[(ch + bits + ms) % 2]
    param = make_parameter(ch, bits, 1024, 48000, ms, trials)
    _, _, spb = ob.geometry(1024, ch, bits)
    rng = np.random.default_rng(ch * 100 + bits * 10 + ms)
    rows = make_rows(rng, ch, lengths_for(spb), types[0], seed=ch * 7 + bits)
    run_stats_case(engine, param, rows, types[0], types[1])


@pytest.mark.parametrize("trials", [0, 2])
@pytest.mark.parametrize("ch,bits,ms", [(1, 4, False), (2, 4, False), (2, 3, True), (2, 2, True), (3, 2, False)])
def test_records_from_the_oracle(engine, ch, bits, ms, trials):
    """the expectation from oracle_binding's encode + decode, not from the library's own rows"""
    import torch
    param = make_parameter(ch, bits, 1024, 48000, ms, trials)
    _, _, spb = ob.geometry(1024, ch, bits)
    rng = np.random.default_rng(ch + bits)
    lengths = [1, 5, 17, spb - 1, spb + 1, 3 * spb + 9]
    for dt in (np.int16, np.float32):
        rows = make_rows(rng, ch, lengths, dt, seed=bits)
        buf, offs, cs = lay_out(rows, ch, dt)
        table, total = image_table(engine, param, lengths)
        table["pcm_offset"] = offs
        plan = engine.planar_reconstruct_plan(param, table, cs, tdt(dt), torch.int16, ch * (max(lengths) + 1), max(lengths) + 1)
        full, stats = stats_table(len(rows), ch, seed=3)
        data = torch.zeros(total, dtype=torch.uint8, device="cuda")
        plan.run(torch.from_numpy(buf).cuda(), data, None, stats=stats)
        torch.cuda.synchronize()
        plan.close()
        check_stats_canaries(full)
        odec = [ob.decode(ob.encode(np.ascontiguousarray(q(r).T), bits, 1024, 48000, ms, trials))[0].T for r in rows]
        assert np.array_equal(stats.cpu().numpy(), expected_stats(rows, odec))


@pytest.mark.parametrize("mapping", ["auto", "dense", "quad", "quad-fused"])
def test_every_mapping(engine, mapping):
    try:
        engine.set_mapping(mapping, "dual")
        rng = np.random.default_rng(5)
        k = 0
        for ch, ms in ((1, False), (2, False), (2, True)):
            for bits in (4, 3, 2):
                for trials in (0, 2):
                    # 40 streams: quad territory under auto; 200 / 3000: dense
                    for streams in (40, 200 if trials == 0 else 3000):
                        param = make_parameter(ch, bits, 1024, 48000, ms, trials)
                        _, _, spb = ob.geometry(1024, ch, bits)
                        lengths = [(spb + 1, 2 * spb, 3, spb - 5, 16, 21)[i % 6] for i in range(streams)]
                        dt = np.float32 if streams % 3 else np.int16
                        rows = make_rows(rng, ch, lengths, dt, seed=streams + bits)
                        run_stats_case(engine, param, rows, dt, (np.float32, np.int16, None)[k % 3], aligned=streams == 200)
                        k += 1
    finally:
        engine.set_mapping("auto", "dual")


@pytest.mark.parametrize("L,W", [(1, 0), (3, 1), (16, 4)])
@pytest.mark.parametrize("types", [(np.int16, np.float32), (np.float32, np.int16), (np.float32, None)], ids=["i16-f32", "f32-i16", "f32-none"])
def test_segmented(engine, L, W, types):
    rng = np.random.default_rng(L * 10 + W)
    for ch, bits, ms, trials in ((2, 4, False, 0), (2, 3, True, 2), (1, 2, False, 2), (3, 4, False, 0), (1, 4, False, 0)):
        param = make_parameter(ch, bits, 1024, 48000, ms, trials)
        _, _, spb = ob.geometry(1024, ch, bits)
        lengths = [40 * spb + 13, 3, spb, 17 * spb, 2 * spb + 1]
        rows = make_rows(rng, ch, lengths, types[0], seed=bits + L)
        run_stats_case(engine, param, rows, types[0], types[1], seg=(L, W))


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
            _, st = run_stats_case(engine, param, rows, dtype, np.float32, state=st)


def test_extreme_inputs(engine):
    """full-scale noise and square waves at 2 bits (clipping, a large max_abs), digital silence (zero sums, the right count), and
    float32 specials - the error is against q(v)"""
    rng = np.random.default_rng(21)
    for ch, ms in ((1, False), (2, False), (2, True)):
        for trials in (0, 2):
            param = make_parameter(ch, 2, 1024, 48000, ms, trials)
            _, _, spb = ob.geometry(1024, ch, 2)
            n = 2 * spb + 37
            noise = rng.integers(-32768, 32768, size=(ch, n)).astype(np.int16)
            square = np.where((np.arange(n) // 3) % 2, 32767, -32768).astype(np.int16)[None, :].repeat(ch, 0).copy()
            if ch == 2:
                square[1] = -1 - square[1]
            silence = np.zeros((ch, n), dtype=np.int16)
            got, _ = run_stats_case(engine, param, [noise, square, silence], np.int16, np.int16, oracle=True)
            assert (got[2, :, :3] == 0).all() and (got[2, :, 3] == n).all()
            assert got[0, :, 2].min() > 16384, "full-scale noise at 2 bits was meant to be hit hard"
            special = np.array(F32_SPECIALS_BITS, dtype=np.uint32).view(np.float32)
            wild = rng.uniform(-3, 3, size=(ch, n)).astype(np.float32)
            wild[:, ::5] = np.resize(special, wild[:, ::5].shape)
            wild[:, 1::97] = np.inf
            wild[:, 2::89] = -np.inf
            wild[:, 3::83] = np.nan
            run_stats_case(engine, param, [wild, silence.astype(np.float32), (noise.astype(np.float32) / 32768)], np.float32,
                           np.float32, oracle=True)


def _create(engine, param, layout, output, seg, table):
    plan = C.c_void_p()
    rc = engine.lib.AADHip_PlanarReconstructPlanCreate(engine._ctx, C.byref(param), C.byref(layout), C.byref(output),
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
    IA, OK = AADApiResult.INVALID_ARGUMENT, AADApiResult.OK
    x = torch.zeros(1000, dtype=torch.float32, device="cuda")
    data = torch.zeros(total, dtype=torch.uint8, device="cuda")
    out = torch.zeros(400, dtype=torch.float32, device="cuda")
    state = torch.zeros((4, 10), dtype=torch.int32, device="cuda")
    stats = torch.zeros(4 * 4 + 1, dtype=torch.int64, device="cuda")
    run = engine.lib.AADHip_PlanarReconstructPlanRunStats
    # a stream without frames cannot be in a plan, so no record is ever an empty row's
    none = table.copy()
    none["num_samples"][1] = 0
    assert _create(engine, param, lay, out_ok, None, none)[0] == AADApiResult.INVALID_FORMAT
    assert _create(engine, param, lay, AADHipPlanarOutput(SAMPLE_FLOAT32, 1, 200, 100), None, table)[0] == IA  # reserved stays refused
    rc, rec = _create(engine, param, lay, out_ok, None, table)
    assert rc == OK
    assert run(rec, None, data.data_ptr(), out.data_ptr(), None, stats.data_ptr()) == IA
    assert run(rec, x.data_ptr(), None, out.data_ptr(), None, stats.data_ptr()) == IA
    assert run(rec, x.data_ptr(), data.data_ptr(), out.data_ptr(), None, None) == IA                       # no table
    assert run(rec, x.data_ptr(), data.data_ptr(), out.data_ptr(), None, stats.data_ptr() + 4) == IA       # misaligned
    assert run(rec, x.data_ptr(), data.data_ptr(), x.data_ptr(), None, stats.data_ptr()) == IA             # out == input
    assert run(None, x.data_ptr(), data.data_ptr(), out.data_ptr(), None, stats.data_ptr()) == IA
    assert run(rec, x.data_ptr(), data.data_ptr(), None, None, stats.data_ptr()) == OK                     # no rows: allowed here
    assert run(rec, x.data_ptr(), data.data_ptr(), out.data_ptr(), state.data_ptr(), stats.data_ptr() + 8) == OK  # 8-byte aligned
    assert engine.lib.AADHip_PlanarReconstructPlanRun(rec, x.data_ptr(), data.data_ptr(), None, None) == IA  # ... and only here
    engine.lib.AADHip_EncodePlanDestroy(rec)
    rc, seg = _create(engine, param, lay, out_ok, AADHipSegmentation(1, 0), table)
    assert rc == OK
    assert run(seg, x.data_ptr(), data.data_ptr(), out.data_ptr(), state.data_ptr(), stats.data_ptr()) == IA
    assert run(seg, x.data_ptr(), data.data_ptr(), out.data_ptr(), None, None) == IA
    assert run(seg, x.data_ptr(), data.data_ptr(), out.data_ptr(), None, stats.data_ptr()) == OK
    engine.lib.AADHip_EncodePlanDestroy(seg)
    planar = engine.planar_encode_plan(param, table, 100, torch.float32)
    assert run(planar.handle, x.data_ptr(), data.data_ptr(), out.data_ptr(), None, stats.data_ptr()) == IA
    planar.close()
    inter = engine.encode_plan(param, table)
    assert run(inter.handle, x.data_ptr(), data.data_ptr(), out.data_ptr(), None, stats.data_ptr()) == IA
    inter.close()
    empty = np.zeros(0, dtype=STREAM_DESC_DTYPE)
    rc, e = _create(engine, param, lay, out_ok, None, empty)
    assert rc == OK and run(e, x.data_ptr(), data.data_ptr(), None, None, None) == OK  # no streams: nothing to write, nothing launched
    engine.lib.AADHip_EncodePlanDestroy(e)
    torch.cuda.synchronize()
    p = engine.planar_reconstruct_plan(param, table, 100, torch.float32, torch.float32, 200, 100)
    with pytest.raises(ValueError, match="stats"):
        p.run(x, data, None)
    with pytest.raises(ValueError, match="stats"):
        p.run(x, data, out, stats=torch.zeros((2, 2, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="stats"):
        p.run(x, data, out, stats=torch.zeros((2, 2, 8), dtype=torch.int64, device="cuda")[:, :, ::2])
    p.close()


@pytest.mark.parametrize("seg", [None, (2, 1)], ids=["serial", "segmented"])
def test_signal_events_and_non_default_stream(engine, seg):
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
        y, stats = eng.reconstruct_planar(x, param, return_stats=True, segment_blocks=seg and seg[0], warmup_blocks=seg[1] if seg else 0)
        stop.synchronize()
        assert start.elapsed_ms(stop) > 0
        # the stop event sits behind the run's last operation: the table is complete once it has fired
        first = stats.clone()
    torch.cuda.synchronize()
    assert torch.equal(first, stats)
    y2 = engine.reconstruct_planar(x, param, segment_blocks=seg and seg[0], warmup_blocks=seg[1] if seg else 0)
    assert torch.equal(y, y2)
    e = q(x.cpu().numpy()).astype(np.int64) - np.round(y.cpu().numpy().astype(np.float64) * 32768).astype(np.int64)
    want = np.stack([(e * e).sum(-1), np.abs(e).sum(-1), np.abs(e).max(-1), np.full(e.shape[:2], e.shape[2])], axis=-1)
    assert np.array_equal(stats.cpu().numpy(), want)
    start.close()
    stop.close()
    eng.close()


def test_engine_calls(engine):
    import torch
    for dtype, ch, ms in ((torch.float32, 2, True), (torch.int16, 2, False), (torch.float32, 3, False), (torch.int16, 1, False)):
        param = make_parameter(ch, 3, 1024, 48000, ms, 2)
        big = torch.randn((7, ch + 1, 5000), device="cuda") * 0.3
        if dtype == torch.int16:
            big = (big * 32768).clamp(-32768, 32767).to(torch.int16)
        x = big[1:6, 1:, 3:3 + 2777]  # stride(1) = 5000 > T, odd element offset
        lengths = [2777, 1, 1500, 4, 2048]
        for seg in (None, (1, 1)):
            kw = dict(num_samples=lengths, segment_blocks=seg and seg[0], warmup_blocks=seg[1] if seg else 0)
            y = engine.reconstruct_planar(x, param, dtype=torch.int16, **kw)
            y1, stats = engine.reconstruct_planar(x, param, dtype=torch.int16, return_stats=True, **kw)
            y2, images, sizes, stats2 = engine.reconstruct_planar(x, param, dtype=torch.float32, return_images=True, return_stats=True, **kw)
            only = engine.codec_error(x, param, **kw)
            assert stats.dtype == torch.int64 and tuple(stats.shape) == (5, ch, 4)
            assert torch.equal(y, y1) and torch.equal(y2, y.to(torch.float32) / 32768)
            assert torch.equal(stats, stats2) and torch.equal(stats, only)
            xq = q(x.cpu().numpy())
            dec = y.cpu().numpy()
            want = expected_stats([xq[i, :, :n] for i, n in enumerate(lengths)], [dec[i, :, :n] for i, n in enumerate(lengths)])
            assert np.array_equal(stats.cpu().numpy(), want)
            if seg is None:
                for i, n in enumerate(lengths):
                    assert np.array_equal(ob.decode(bytes(images[i, :sizes[i]].cpu().numpy()))[0].T, dec[i, :, :n])


def test_least_bits_differs_from_row_to_row(engine):
    """silence, a quiet sine, a loud sine, full-scale noise, low-passed noise and a stream whose second channel is the hard one: the
    fewest bits that keep 25 dB come out as 2, 0, 2, 0, 3, 4; against the same selection made in numpy from oracle encodes and
    decodes"""
    import torch
    from aad_amd.engine import snr_db
    n, ch = 6000, 2
    t = np.arange(n)
    rng = np.random.default_rng(2)
    rows = np.zeros((6, ch, n), dtype=np.float32)
    rows[1] = 0.01 * np.sin(2 * np.pi * t / 97.0)
    rows[2] = 0.8 * np.sin(2 * np.pi * t / 41.0)
    rows[3] = rng.uniform(-1, 1, size=(ch, n))
    rows[4] = 2 * np.convolve(rng.standard_normal(n + 39), np.ones(40) / 40, "valid")  # noise below 600 Hz
    rows[5, 0] = rows[2, 0]
    rows[5, 1] = 0.5 * np.sin(2 * np.pi * t / 60.0) + 0.1 * rng.standard_normal(n)  # one hard channel decides for the stream
    lengths = [n, n, n - 7, n, n, n]
    make = lambda bits: make_parameter(ch, bits, 1024, 48000, False, 2)  # noqa: E731
    x = torch.from_numpy(rows).cuda()
    snrs = []
    for bits in (2, 3, 4):
        snr = np.zeros((len(lengths), ch))
        for i, m in enumerate(lengths):
            pcm = q(rows[i, :, :m])
            dec = ob.decode(ob.encode(np.ascontiguousarray(pcm.T), bits, 1024, 48000, False, 2))[0].T
            e = (pcm.astype(np.int64) - dec.astype(np.int64))
            sig, err = (pcm.astype(np.int64) ** 2).sum(-1), (e * e).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                snr[i] = np.where(err == 0, np.inf, 10 * np.log10(sig / np.maximum(err, 1)))
        snrs.append(snr)
        signal = torch.from_numpy(np.stack([(q(rows[i, :, :m]).astype(np.int64) ** 2).sum(-1) for i, m in enumerate(lengths)])).cuda()
        got = snr_db(engine.codec_error(x, make(bits), num_samples=lengths), signal).cpu().numpy()
        assert np.allclose(got, snr, rtol=1e-12, atol=0, equal_nan=True), "snr_db at %d bits" % bits  # same integers, one log10 apart
    for bound in (30.0, 25.0):
        want = np.zeros(len(lengths), dtype=np.int64)
        for bits, snr in reversed(list(zip((2, 3, 4), snrs))):
            want = np.where((snr >= bound).all(-1), bits, want)
        got = engine.least_bits(x, make, bound, num_samples=lengths)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (bound, got, want)
    assert set(want.tolist()) == {0, 2, 3, 4}, "the rows were built so that every answer occurs at 25 dB: %s" % (want,)
