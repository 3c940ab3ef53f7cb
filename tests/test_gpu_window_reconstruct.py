"""Window reconstruct on the device (AADHip_WindowReconstructPlanRun, WindowReconstructPlan.run, Engine.reconstruct_windows,
Engine.codec_error_windows): crops named by a window table in device memory, read where they lie in a PCM corpus and run through
the encoders.

Bar (include/aad_hip.h "window reconstruct"): == on every byte, every row element and every integer of every record.  Expected
values come from the pinned oracle: for a window with len_w > 0, ob.encode of the host-gathered crop is the image, ob.decode of
that image / 32768 the rows, and numpy int64 arithmetic on q(x) - decoded the statistics.  Segmented cases are compared with
Engine.reconstruct_planar(..., num_samples=len, segment_blocks, warmup_blocks, return_images, return_stats) on the gathered crops,
which tests/test_gpu_planar_reconstruct.py and tests/test_gpu_planar_stats.py hold to the oracle.  A window with len_w == 0 gives
the 31-byte header with num_samples = 0, zero rows and zero records.  Canaries surround every image slot, every row and the
statistics table; rows are zero from len_w to T; the input must be unchanged.

Source: six streams of {1, 37, spb, 3 spb + 5, 5 spb + 77, 0} frames at odd offsets, channel_stride above the longest; block size
256, T = 3 spb + 11 (four blocks)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle_binding as ob
from aad_amd.capi import AADApiResult, AADHipPlanarLayout, AADHipPlanarOutput, AADHipSegmentation, SAMPLE_FLOAT32, SAMPLE_INT16, \
    STREAM_DESC_DTYPE, make_parameter
from test_gpu_planar_encode import CANARY, lay_out, make_rows, q
from test_gpu_planar_reconstruct import out_buffer, tdt
from test_gpu_planar_stats import check_stats_canaries, expected_stats, stats_table

pytestmark = pytest.mark.gpu

BLOCK = 256
U64 = (1 << 64) - 1
BASE, ROW_PAD, STREAM_PAD, IMAGE_PAD, IMAGE_LEAD = 7, 5, 13, 17, 24


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def source_lengths(spb):
    return [1, 37, spb, 3 * spb + 5, 5 * spb + 77, 0]


def window_list(spb, frames):
    n = source_lengths(spb)
    s = len(n)
    return [(3, 0), (4, 0),                                  # starts at 0
            (4, spb // 2 + 3), (3, 7), (4, spb + 1),         # mid-block starts
            (4, n[4] - frames), (4, n[4] - frames - 1),      # ending exactly at n_s, and one frame before
            (4, n[4] - frames + 1), (4, n[4] - 1),           # past the end by 1 and by T - 1
            (3, n[3]), (3, n[3] + 1), (0, 1), (0, 2),        # starts at n_s and n_s + 1
            (5, 0), (5, 3),                                  # the empty source stream
            (s, 0), (U64, 0), (0, U64), (U64, U64), (3, 1 << 63),
            (2, 0), (2, spb - 1), (1, 0), (1, 36), (0, 0),   # streams of a block and less
            (4, 2 * spb), (4, 0)]                            # ... and the same window twice


def window_length(lengths, stream, first, frames):
    if stream >= len(lengths) or first >= lengths[stream]:
        return 0
    return min(frames, lengths[stream] - first)


_sources = {}


def source(ch, bits, dtype):
    """the corpus of a geometry and sample type, made once: (rows per stream, flat buffer, offsets, channel_stride)"""
    key = (ch, bits, np.dtype(dtype).name)
    if key not in _sources:
        lengths = source_lengths(ob.geometry(BLOCK, ch, bits)[1])
        rows = make_rows(np.random.default_rng(5), ch, [max(v, 1) for v in lengths], dtype, seed=11)
        rows = [r[:, :v] for r, v in zip(rows, lengths)]
        _sources[key] = (rows,) + lay_out(rows, ch, dtype)
    return _sources[key]


_expected = {}


def expected(engine, ch, bits, ms, trials, dtype, seg):
    """per window (len, image bytes, decoded int16 [C, len], records [C, 4]) - computed once per codec setting and shared"""
    key = (ch, bits, ms, trials, np.dtype(dtype).name, seg)
    if key in _expected:
        return _expected[key]
    import torch
    rows, _, _, _ = source(ch, bits, dtype)
    lengths = [r.shape[1] for r in rows]
    spb = ob.geometry(BLOCK, ch, bits)[1]
    frames = 3 * spb + 11
    wins = window_list(spb, frames)
    crops = []
    for s, f in wins:
        n = window_length(lengths, s, f, frames)
        crops.append(rows[s][:, f:f + n] if n else np.zeros((ch, 0), dtype=dtype))
    live = [i for i, c in enumerate(crops) if c.shape[1]]
    result = [None] * len(wins)
    if seg is None:
        header = None
        for i in live:
            img = ob.encode(np.ascontiguousarray(q(crops[i]).T), bits, BLOCK, 48000, ms, trials)
            dec = np.ascontiguousarray(ob.decode(img)[0].T)
            result[i] = (crops[i].shape[1], bytes(img), dec, expected_stats([crops[i]], [dec])[0])
            header = bytes(img[:31])
    else:
        param = make_parameter(ch, bits, BLOCK, 48000, ms, trials)
        x = np.zeros((len(live), ch, frames), dtype=dtype)
        for k, i in enumerate(live):
            x[k, :, :crops[i].shape[1]] = crops[i]
        y, images, sizes, stats = engine.reconstruct_planar(torch.from_numpy(x).cuda(), param, num_samples=[crops[i].shape[1] for i in live],
                                                            dtype=torch.int16, segment_blocks=seg[0], warmup_blocks=seg[1],
                                                            return_images=True, return_stats=True)
        torch.cuda.synchronize()
        y, images, stats = y.cpu().numpy(), images.cpu().numpy(), stats.cpu().numpy()
        for k, i in enumerate(live):
            n = crops[i].shape[1]
            result[i] = (n, bytes(images[k, :sizes[k]]), y[k, :, :n].copy(), stats[k].copy())
        header = bytes(images[0, :31])
    empty = header[:14] + bytes(4) + header[18:]
    for i in range(len(wins)):
        if result[i] is None:
            result[i] = (0, empty, np.zeros((ch, 0), dtype=np.int16), np.zeros((ch, 4), dtype=np.int64))
    _expected[key] = (wins, frames, result)
    return _expected[key]


def windows_tensor(wins):
    import torch
    return torch.from_numpy(np.array(wins, dtype=np.uint64).reshape(-1, 2).view(np.int64)).cuda()


def strided_rows(n, ch, frames, out_dtype):
    """[n, ch, frames] view, strides (oss, ocs, 1), inside a canary-filled buffer"""
    import torch
    ocs = frames + ROW_PAD
    oss = ch * ocs + STREAM_PAD
    full = out_buffer(BASE + n * oss + 11, out_dtype)
    return full, torch.as_strided(full, (n, ch, frames), (oss, ocs, 1), BASE)


def check_rows(full, n, ch, frames, out_dtype, result):
    ocs = frames + ROW_PAD
    oss = ch * ocs + STREAM_PAD
    got = full.cpu().numpy()
    want = out_buffer(BASE + n * oss + 11, out_dtype).cpu().numpy()
    for w in range(n):
        length, _, dec, _ = result[w]
        for c in range(ch):
            row = np.zeros(frames, dtype=np.int16)
            row[:length] = dec[c]
            at = BASE + w * oss + c * ocs
            want[at:at + frames] = row.astype(np.float32) / np.float32(32768) if out_dtype == np.float32 else row
    bits = np.uint32 if out_dtype == np.float32 else np.uint16
    bad = np.flatnonzero(got.view(bits) != want.view(bits))
    if bad.size:
        at = int(bad[0]) - BASE
        pytest.fail("rows: element %d of window %d differs (offset %d in its slot, %d elements differ): got %r, want %r"
                    % (int(bad[0]), at // oss, at % oss, bad.size, got[bad[0]], want[bad[0]]))


def check_images(data, n, stride, result):
    got = data.cpu().numpy()
    want = np.full(got.shape, CANARY, dtype=np.uint8)
    for w in range(n):
        img = result[w][1]
        want[IMAGE_LEAD + w * stride:IMAGE_LEAD + w * stride + len(img)] = np.frombuffer(img, dtype=np.uint8)
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = int(bad[0]) - IMAGE_LEAD
        pytest.fail("images: byte %d of window %d's slot (len_w %d, image of %d bytes) differs, %d bytes differ"
                    % (at % stride, at // stride, result[at // stride][0], len(result[at // stride][1]), bad.size))


def run_case(engine, ch, bits, ms=False, trials=0, in_dtype=np.float32, out_dtype=np.float32, seg=None,
             subset=("images", "rows", "stats"), mapping="auto"):
    import torch
    wins, frames, result = expected(engine, ch, bits, ms, trials, in_dtype, seg)
    n = len(wins)
    rows, buf, offs, cs = source(ch, bits, in_dtype)
    table = np.zeros(len(rows), dtype=STREAM_DESC_DTYPE)
    table["pcm_offset"] = offs
    table["num_samples"] = [r.shape[1] for r in rows]
    table["data_offset"], table["data_size"] = 0xDEAD, 3  # ignored
    param = make_parameter(ch, bits, BLOCK, 48000, ms, trials)
    x = torch.from_numpy(buf).cuda()
    w = windows_tensor(wins)
    stride = engine.encoded_size(param, frames) + IMAGE_PAD
    engine.set_mapping(mapping)
    try:
        plan = engine.window_reconstruct_plan(param, table, cs, tdt(in_dtype), *(seg or (None, 0)))
        full_rows, out = strided_rows(n, ch, frames, out_dtype) if "rows" in subset else (None, False)
        data = torch.full((IMAGE_LEAD + n * stride + 40,), CANARY, dtype=torch.uint8, device="cuda") if "images" in subset else None
        full_stats, stats = stats_table(n, ch, seed=3) if "stats" in subset else (None, None)
        slots = None if data is None else torch.as_strided(data, (n, stride), (stride, 1), IMAGE_LEAD)
        plan.run(x, w, frames, out=out, data=slots, stats=stats)
        torch.cuda.synchronize()
        plan.close()
    finally:
        engine.set_mapping("auto")
    assert np.array_equal(x.cpu().numpy().view(np.uint8), buf.view(np.uint8)), "the corpus changed"
    assert np.array_equal(w.cpu().numpy().view(np.uint64).reshape(-1), np.array(wins, dtype=np.uint64).reshape(-1)), "the windows changed"
    if data is not None:
        check_images(data, n, stride, result)
    if full_rows is not None:
        check_rows(full_rows, n, ch, frames, out_dtype, result)
    if stats is not None:
        check_stats_canaries(full_stats)
        got, want = stats.cpu().numpy(), np.stack([r[3] for r in result])
        bad = np.argwhere(got != want)
        if bad.size:
            i, c, f = (int(v) for v in bad[0])
            pytest.fail("window %d %r (len_w %d) channel %d field %d: got %d, want %d" % (i, wins[i], result[i][0], c, f, got[i, c, f], want[i, c, f]))


def test_the_window_list_covers_the_edges():
    spb = ob.geometry(BLOCK, 2, 4)[1]
    frames = 3 * spb + 11
    lengths = source_lengths(spb)
    wins = window_list(spb, frames)
    lens = [window_length(lengths, s, f, frames) for s, f in wins]
    assert -(-frames // spb) >= 4 and 20 <= len(wins) <= 30
    assert frames in lens and 0 in lens and 1 in lens and frames - 1 in lens and any(0 < v < spb for v in lens)
    assert len(set(wins)) < len(wins)


@pytest.mark.parametrize("ch,bits", [(ch, bits) for ch in (1, 2, 3) for bits in (2, 3, 4)])
@pytest.mark.parametrize("seg", [None, (1, 0), (2, 1)], ids=["serial", "L1W0", "L2W1"])
def test_channels_bits_and_segmentations(engine, ch, bits, seg):
    run_case(engine, ch, bits, seg=seg)


@pytest.mark.parametrize("seg", [None, (2, 1)], ids=["serial", "L2W1"])
@pytest.mark.parametrize("trials", [0, 2])
def test_mid_side_and_trials(engine, trials, seg):
    run_case(engine, 2, 4, ms=True, trials=trials, seg=seg)
    if trials:
        run_case(engine, 2, 4, trials=trials, seg=seg)
        run_case(engine, 1, 3, trials=trials, seg=seg, in_dtype=np.int16)


@pytest.mark.parametrize("in_dtype,out_dtype", list(itertools.product([np.int16, np.float32], repeat=2)), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("seg", [None, (2, 1)], ids=["serial", "L2W1"])
def test_sample_type_pairs(engine, in_dtype, out_dtype, seg):
    run_case(engine, 2, 4, in_dtype=in_dtype, out_dtype=out_dtype, seg=seg)
    run_case(engine, 1, 4, in_dtype=in_dtype, out_dtype=out_dtype, seg=seg)  # mono int16 rows are the interleaved layout


@pytest.mark.parametrize("mapping", ["auto", "dense", "quad"])
@pytest.mark.parametrize("seg", [None, (1, 0), (2, 1)], ids=["serial", "L1W0", "L2W1"])
def test_lane_mappings(engine, mapping, seg):
    for trials in (0, 2):
        run_case(engine, 2, 4, trials=trials, seg=seg, mapping=mapping)
    run_case(engine, 1, 2, seg=seg, mapping=mapping, in_dtype=np.int16, out_dtype=np.int16)


SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(("images", "rows", "stats"), k)]


@pytest.mark.parametrize("subset", SUBSETS, ids=["+".join(s) for s in SUBSETS])
@pytest.mark.parametrize("seg", [None, (2, 1)], ids=["serial", "L2W1"])
def test_every_subset_of_the_outputs(engine, subset, seg):
    for trials in (0, 2):  # images alone run the plain planar encoders, whose trial search has a lane layout of its own
        run_case(engine, 2, 4, trials=trials, seg=seg, subset=subset)
    run_case(engine, 1, 4, seg=seg, subset=subset, in_dtype=np.int16, out_dtype=np.int16)


def gather_reference(engine, corpus, wins, frames, param, dtype, **kw):
    """the composite the feature replaces: crops gathered on the host side of torch, then reconstruct_planar"""
    import torch
    s, ch, t = corpus.shape
    x = torch.zeros((len(wins), ch, frames), dtype=corpus.dtype, device="cuda")
    lens = []
    for i, (r, f) in enumerate(wins):
        n = max(0, min(frames, t - f)) if 0 <= r < s else 0
        lens.append(n)
        if n:
            x[i, :, :n] = corpus[r, :, f:f + n]
    live = [i for i, n in enumerate(lens) if n]
    y, stats = engine.reconstruct_planar(x[live], param, num_samples=[lens[i] for i in live], dtype=dtype, return_stats=True, **kw)
    full_y = torch.zeros((len(wins), ch, frames), dtype=dtype, device="cuda")
    full_s = torch.zeros((len(wins), ch, 4), dtype=torch.int64, device="cuda")
    full_y[live], full_s[live] = y, stats
    return full_y, full_s


@pytest.mark.parametrize("seg", [None, (2, 1)], ids=["serial", "L2W1"])
def test_windows_drawn_on_the_device_on_a_side_stream(seg):
    import torch
    from aad_amd.engine import Engine
    param = make_parameter(2, 4, BLOCK, 48000, False, 0)
    kw = dict(segment_blocks=seg[0], warmup_blocks=seg[1]) if seg else {}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng = Engine(0)
        assert eng.stream.cuda_stream == side.cuda_stream
        g = torch.Generator(device="cuda").manual_seed(7)
        corpus = (torch.randn((5, 2, 1500), device="cuda", generator=g) * 0.3)[:, :, 3:1403]  # a view: rows at odd offsets
        wins = torch.stack([torch.randint(0, 6, (70,), device="cuda", generator=g),              # stream 5 does not exist
                            torch.randint(0, 1500, (70,), device="cuda", generator=g)], dim=1)  # queued, not yet run
        y, stats = eng.reconstruct_windows(corpus, wins, 400, param, return_stats=True, **kw)
        only = eng.codec_error_windows(corpus, wins, 400, param, **kw)
        y16, images, stride = eng.reconstruct_windows(corpus, wins, 400, param, dtype=torch.int16, return_images=True, **kw)
    torch.cuda.synchronize()
    host = [(int(a), int(b)) for a, b in wins.cpu().numpy()]
    want_y, want_s = gather_reference(eng, corpus, host, 400, param, torch.float32, **kw)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), want_y.view(torch.int32)) and torch.equal(stats, want_s) and torch.equal(only, want_s)
    assert torch.equal(y16.to(torch.float32) / 32768, want_y)
    counts = images[:, 14:18].cpu().numpy().astype(np.int64)
    assert np.array_equal((counts[:, 0] << 24) | (counts[:, 1] << 16) | (counts[:, 2] << 8) | counts[:, 3], want_s[:, 0, 3].cpu().numpy())
    assert stride >= eng.encoded_size(param, 400) and (want_s[:, 0, 3] == 0).any() and (want_s[:, 0, 3] == 400).any()
    eng.close()


def test_no_windows_and_one_plan_for_any_run(engine):
    import torch
    rows, buf, offs, cs = source(2, 4, np.float32)
    table = np.zeros(len(rows), dtype=STREAM_DESC_DTYPE)
    table["pcm_offset"], table["num_samples"] = offs, [r.shape[1] for r in rows]
    param = make_parameter(2, 4, BLOCK, 48000, False, 0)
    x = torch.from_numpy(buf).cuda()
    for seg in (None, (2, 1)):
        plan = engine.window_reconstruct_plan(param, table, cs, torch.float32, *(seg or (None, 0)))
        y = plan.run(x, torch.zeros((0, 2), dtype=torch.int64, device="cuda"), 100)
        assert tuple(y.shape) == (0, 2, 100)
        wins, frames, result = expected(engine, 2, 4, False, 0, np.float32, seg)
        # a short run first, then one that outgrows the plan's tables, with another T and output type
        few = plan.run(x, windows_tensor(wins[:3]), frames, dtype=torch.float32)
        stats = torch.empty((len(wins), 2, 4), dtype=torch.int64, device="cuda")
        many = plan.run(x, windows_tensor(wins), frames, dtype=torch.int16, stats=stats)
        short = plan.run(x, windows_tensor(wins), 50, dtype=torch.int16)
        torch.cuda.synchronize()
        plan.close()
        many, few, short = many.cpu().numpy(), few.cpu().numpy(), short.cpu().numpy()
        for i, (n, _, dec, rec) in enumerate(result):
            assert np.array_equal(many[i, :, :n], dec) and not many[i, :, n:].any()
            assert np.array_equal(stats[i].cpu().numpy(), rec)
            if i < 3:
                assert np.array_equal(few[i, :, :n], dec.astype(np.float32) / np.float32(32768))
        # T = 50 lies inside the first block, which every chain cut encodes like the serial encoder: the first 50 decoded samples
        lengths = [r.shape[1] for r in rows]
        for i, (s, f) in enumerate(wins):
            n = window_length(lengths, s, f, 50)
            crop = rows[s][:, f:f + n] if n else None
            if n:
                dec = ob.decode(ob.encode(np.ascontiguousarray(q(crop).T), 4, BLOCK, 48000, False, 0))[0].T
                assert np.array_equal(short[i, :, :n], dec)
            assert not short[i, :, n:].any()


def test_signal_events_around_a_segmented_run_with_statistics(engine):
    import torch
    from aad_amd.engine import HipEvent
    wins, frames, result = expected(engine, 2, 4, False, 0, np.float32, (2, 1))
    rows, buf, offs, cs = source(2, 4, np.float32)
    table = np.zeros(len(rows), dtype=STREAM_DESC_DTYPE)
    table["pcm_offset"], table["num_samples"] = offs, [r.shape[1] for r in rows]
    plan = engine.window_reconstruct_plan(make_parameter(2, 4, BLOCK, 48000, False, 0), table, cs, torch.float32, 2, 1)
    x, w = torch.from_numpy(buf).cuda(), windows_tensor(wins)
    stats = torch.full((len(wins), 2, 4), -7, dtype=torch.int64, device="cuda")
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    engine.signal_next(stop, start=start)
    y = plan.run(x, w, frames, stats=stats)
    stop.synchronize()
    assert start.elapsed_ms(stop) > 0
    first = (y.clone(), stats.clone())  # the stop event sits behind the run's last operation: rows and table are complete
    torch.cuda.synchronize()
    assert torch.equal(first[0], y) and torch.equal(first[1], stats)
    assert np.array_equal(stats.cpu().numpy(), np.stack([r[3] for r in result]))
    # one-shot: the next run takes no events, and withdrawing is fine
    plan.run(x, w, frames, stats=stats)
    torch.cuda.synchronize()
    plan.close()


def test_api_errors_and_cross_use(engine):
    import torch
    lib, ctx = engine.lib, engine._ctx
    INV = AADApiResult.INVALID_ARGUMENT
    param = make_parameter(2, 4, BLOCK, 48000, False, 0)
    spb = ob.geometry(BLOCK, 2, 4)[1]
    frames = 3 * spb + 11
    size = engine.encoded_size(param, frames)
    src = np.zeros(2, dtype=STREAM_DESC_DTYPE)
    src["pcm_offset"], src["num_samples"] = [0, 5000], [2000, 1000]
    plan = C.c_void_p()

    def create(p=param, layout=AADHipPlanarLayout(SAMPLE_FLOAT32, 0, 2000), seg=None, table=src):
        return lib.AADHip_WindowReconstructPlanCreate(ctx, C.byref(p), C.byref(layout), C.byref(seg) if seg is not None else None,
                                                      len(table), table.ctypes.data, C.byref(plan))

    assert create(layout=AADHipPlanarLayout(2, 0, 2000)) == INV               # unknown sample type
    assert create(layout=AADHipPlanarLayout(SAMPLE_INT16, 1, 2000)) == INV    # reserved
    assert create(layout=AADHipPlanarLayout(SAMPLE_FLOAT32, 0, 1999)) == INV  # channel_stride below the longest n_s
    assert create(seg=AADHipSegmentation(0, 0)) == INV
    far = src.copy()
    far["pcm_offset"][1] = (1 << 62) - 100
    assert create(table=far) == INV                                           # float32 bytes of a source row past 2^64
    assert create(p=make_parameter(2, 5, BLOCK, 48000, False, 0)) == AADApiResult.INVALID_FORMAT
    assert create(p=make_parameter(1, 4, BLOCK, 48000, True, 0)) == AADApiResult.INVALID_FORMAT
    assert create() == AADApiResult.OK and plan.value
    h = plan.value

    n = 3
    x = torch.zeros(8000, dtype=torch.float32, device="cuda")
    w = torch.zeros((n + 1, 2), dtype=torch.int64, device="cuda")
    data = torch.zeros(n * size + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, 2, frames), dtype=torch.float32, device="cuda")
    stats = torch.zeros((n + 1, 2, 4), dtype=torch.int64, device="cuda")
    good = AADHipPlanarOutput(SAMPLE_FLOAT32, 0, 2 * frames, frames)

    def run(handle=h, samples=x.data_ptr(), count=n, windows=w.data_ptr(), t=frames, stride=size, images=data.data_ptr(),
            output=good, rows=out.data_ptr(), table=stats.data_ptr()):
        return lib.AADHip_WindowReconstructPlanRun(handle, samples, count, windows, t, stride, images,
                                                   C.byref(output) if output is not None else None, rows, table)

    assert run() == AADApiResult.OK
    assert run(t=0) == INV
    assert run(stride=size - 1) == INV and run(stride=size - 1, count=1) == AADApiResult.OK
    assert run(stride=1 << 63) == INV
    assert run(images=None, rows=None, table=None) == INV
    assert run(output=None) == INV and run(output=None, rows=None) == AADApiResult.OK
    assert run(output=AADHipPlanarOutput(2, 0, 2 * frames, frames)) == INV
    assert run(output=AADHipPlanarOutput(SAMPLE_INT16, 7, 2 * frames, frames)) == INV
    assert run(output=AADHipPlanarOutput(SAMPLE_FLOAT32, 0, 2 * frames, frames - 1)) == INV   # channel rows overlap
    assert run(output=AADHipPlanarOutput(SAMPLE_FLOAT32, 0, 2 * frames - 1, frames)) == INV   # windows' rows overlap
    assert run(output=AADHipPlanarOutput(SAMPLE_FLOAT32, 0, 1 << 62, frames)) == INV          # past 64 bits of bytes
    assert run(count=1 << 32, windows=w.data_ptr(), images=None, rows=None) == INV             # lanes
    assert run(windows=None) == INV and run(windows=w.data_ptr() + 4) == INV
    assert run(table=stats.data_ptr() + 4) == INV
    assert run(samples=None) == INV
    assert run(rows=x.data_ptr()) == INV                                                       # device_out == device_samples
    assert run(count=0, windows=None, samples=None) == AADApiResult.OK
    assert run(handle=None) == INV
    torch.cuda.synchronize()
    assert "window reconstruct" in engine.last_error()

    # every other run refuses the window plan, and the window run every other plan
    state = None
    assert lib.AADHip_EncodePlanRun(h, x.data_ptr(), data.data_ptr(), state) == INV
    assert lib.AADHip_PlanarEncodePlanRun(h, x.data_ptr(), data.data_ptr(), state) == INV
    assert lib.AADHip_PlanarReconstructPlanRun(h, x.data_ptr(), data.data_ptr(), out.data_ptr(), state) == INV
    assert lib.AADHip_PlanarReconstructPlanRunStats(h, x.data_ptr(), data.data_ptr(), out.data_ptr(), state, stats.data_ptr()) == INV
    d = np.zeros(1, dtype=STREAM_DESC_DTYPE)
    d["data_size"], d["num_samples"] = size, frames
    others = [engine.encode_plan(param, d), engine.planar_encode_plan(param, d, frames, torch.float32),
              engine.planar_reconstruct_plan(param, d, frames, torch.float32, torch.float32, 2 * frames, frames),
              engine.planar_reconstruct_plan(param, d, frames, torch.float32, torch.float32, 2 * frames, frames, 2, 1)]
    for other in others:
        assert run(handle=other.handle) == INV
        other.close()
    lib.AADHip_WindowReconstructPlanDestroy(h)
    lib.AADHip_WindowReconstructPlanDestroy(None)
