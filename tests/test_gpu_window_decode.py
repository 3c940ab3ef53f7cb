"""Window decode on the device (AADHip_WindowDecodePlanRun, aad_amd/csrc/aad_decode_window.hip.h): crops [first_frame,
first_frame + T) of many streams into planar [N, C, T] rows, int16 and float32.

Bar: bit-exact against the definition (include/aad_hip.h "window decode", restated in tests/window_oracle.py) over
  * images an encoder wrote: slices of tests/oracle_binding.decode - channels 1, 2, 3 and 8, bits 2 / 3 / 4, M/S on and off,
    trials 0 and 2, with the file header and as bare block runs;
  * windows at a block start, mid-block, inside one block, across many blocks, T = 1, the whole stream, ending exactly at the
    stream's end and running past it, starting past it, huge and wrapped-negative values, stream indices out of range;
  * images past a 4 GiB data offset;
  * the crafted streams of tests/golden/bitstream_fuzz.json (truncated images, inconsistent header geometry) against slices of
    AADHip_DecodePlanRun's output, which tests/test_gpu_bitstream_fuzz.py pins to the compiled reference's hashes;
  * images written by a segmented encode.
float32 output is int16 / 32768 bitwise.  API: ordering on a non-default torch stream, windows from torch.randint with no host
synchronisation, AADHip_ContextSignalNextRun events around a run, the run's argument errors."""
import ctypes as C

import numpy as np
import pytest

import bitstream_fuzz as bf
import oracle_binding as ob
from aad_amd.capi import AADApiResult, SAMPLE_FLOAT32, SAMPLE_INT16, STREAM_DESC_DTYPE, make_parameter
from aad_amd.engine import parse_header
from aad_amd.synth import synth_pcm
from window_oracle import window_expected

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A
U64 = 1 << 64


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _pack(images, phase=37, pitch_align=64, base=0):
    """images at odd offsets in one buffer -> (uint8 array, STREAM_DESC_DTYPE table of whole images)"""
    table = np.zeros(len(images), dtype=STREAM_DESC_DTYPE)
    pos = base + phase
    for i, img in enumerate(images):
        table["data_offset"][i] = pos
        table["data_size"][i] = len(img)
        table["num_samples"][i] = parse_header(img[:31]).num_samples
        pos += -(-(len(img) + 5) // pitch_align) * pitch_align + 3
    flat = np.zeros(pos + 64 - base, dtype=np.uint8)
    for i, img in enumerate(images):
        o = int(table["data_offset"][i]) - base
        flat[o:o + len(img)] = np.frombuffer(img, dtype=np.uint8)
    return flat, table


def _bare(table):
    """the same streams as runs of bare blocks (has_file_header = 0): the file header skipped"""
    t = table.copy()
    t["data_offset"] += 31
    t["data_size"] -= 31
    return t


def _windows_for(lengths, spb, frames):
    n0 = lengths[0]
    s_last = len(lengths) - 1
    n_last = lengths[-1]
    rows = [
        (0, 0), (0, spb), (0, 2 * spb), (0, spb + 37), (0, 5), (0, spb - 1),  # block starts, mid-block
        (0, max(n0 - frames, 0)), (0, max(n0 - frames // 2, 0)), (0, n0 - 1),  # ending at / running past the end
        (0, n0), (0, n0 + 5), (0, 1 << 40), (0, -1), (0, -(1 << 62)),        # starting past the end, huge, wrapped
        (len(lengths), 0), ((1 << 63) - 1, 7), (-1, 0),                        # stream out of range
        (s_last, max(n_last - frames, 0)), (s_last, 0), (s_last, n_last // 2),
    ]
    for s, n in enumerate(lengths):
        rows += [(s, 0), (s, (n * 3) // 7), (s, max(n - frames, 0))]
    return np.array(rows, dtype=np.int64)


def _run(torch, plan, d_img, windows_np, frames, channels, dtype):
    """window run into a canary-bordered buffer; returns the [N, C, T] numpy result and checks the border"""
    n = len(windows_np)
    count = n * channels * frames
    big = torch.full((count + 32,), CANARY if dtype == torch.int16 else -7.0, dtype=dtype, device="cuda")
    out = big[16:16 + count].view(n, channels, frames)
    d_win = torch.from_numpy(windows_np).cuda()
    got = plan.run(d_img, d_win, frames, dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = big.cpu().numpy()
    border = np.concatenate([host[:16], host[16 + count:]])
    assert (border == (CANARY if dtype == torch.int16 else -7.0)).all(), "wrote outside its rows"
    return host[16:16 + count].reshape(n, channels, frames)


def _check(torch, plan, d_img, decoded, windows_np, frames, channels, label):
    want16 = window_expected(decoded, windows_np, frames, channels)
    got16 = _run(torch, plan, d_img, windows_np, frames, channels, torch.int16)
    if not np.array_equal(got16, want16):
        w, c, t = [int(v) for v in np.argwhere(got16 != want16)[0]]
        raise AssertionError((label, frames, "window", w, windows_np[w].tolist(), "channel", c, "t", t,
                              got16[w, c, t:t + 4].tolist(), want16[w, c, t:t + 4].tolist()))
    got32 = _run(torch, plan, d_img, windows_np, frames, channels, torch.float32)
    want32 = want16.astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(got32.view(np.uint32), want32.view(np.uint32)), (label, frames, "float32 is not int16 / 32768")


# (channels, bits, ms)
GEOMETRIES = [(c, b, False) for c in (1, 2, 3, 8) for b in (4, 3, 2)] + [(2, b, True) for b in (4, 3, 2)]


@pytest.mark.parametrize("trials", [0, 2])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dch%db%s" % (g[0], g[1], "ms" if g[2] else ""))
def test_windows_equal_slices_of_the_oracle_decode(engine, geometry, trials):
    import torch
    channels, bits, ms = geometry
    lengths = [5003, 12345, 777, 1]
    images, decoded = [], []
    for i, n in enumerate(lengths):
        pcm = synth_pcm(1, n, channels, seed=100 + 7 * i + channels * 31 + bits)[0]
        img = ob.encode(pcm, bits, 1024, 48000, ms, trials)
        images.append(img)
        decoded.append(ob.decode(img)[0])
    hd = parse_header(images[0][:31])
    spb = hd.num_samples_per_block
    flat, table = _pack(images)
    d_img = torch.from_numpy(flat).cuda()
    for with_header, t in ((True, table), (False, _bare(table))):
        plan = engine.window_decode_plan(hd, t, with_header)
        try:
            for frames in sorted({1, 16, 100, spb - 1, spb, spb + 1, 3 * spb + 5, 5003, 12345}):
                _check(torch, plan, d_img, decoded, _windows_for(lengths, spb, frames), frames, channels,
                       (geometry, trials, with_header))
        finally:
            plan.close()


def test_images_past_4gib_offset(engine):
    import torch
    free, _ = torch.cuda.mem_get_info()
    need = (1 << 32) + (64 << 20)
    if free < need + (8 << 30):
        pytest.skip("needs %d GiB of free device memory" % ((need >> 30) + 8))
    images, decoded = [], []
    for i, (ch, n) in enumerate([(2, 30011), (2, 20000), (2, 9999)]):
        pcm = synth_pcm(1, n, ch, seed=900 + i)[0]
        img = ob.encode(pcm, 4, 1024)
        images.append(img)
        decoded.append(ob.decode(img)[0])
    hd = parse_header(images[0][:31])
    base = (1 << 32) - 12000  # the first image straddles byte 2^32, the others lie wholly above it
    flat, table = _pack(images, base=base)
    buf = torch.zeros(base + len(flat), dtype=torch.uint8, device="cuda")
    buf[base:] = torch.from_numpy(flat).cuda()
    try:
        plan = engine.window_decode_plan(hd, table, True)
        for frames in (1, 999, 4800, 30011):
            _check(torch, plan, buf, decoded, _windows_for([30011, 20000, 9999], hd.num_samples_per_block, frames), frames, 2, "4 GiB")
        plan.close()
    finally:
        del buf
        torch.cuda.empty_cache()


def _golden_groups():
    groups = {}
    for rec in bf.golden_cases():
        key = (rec["channels"], rec["bits"], rec["ms"], rec["block_size"], rec["spb"])
        groups.setdefault(key, []).append(rec)
    return groups


def test_crafted_streams_equal_slices_of_decode_plan_run(engine):
    """the golden crafted images (bitstream_fuzz.json: random headers and bodies, ragged last blocks, truncated images,
    inconsistent block_size / samples_per_block) - windows == slices of AADHip_DecodePlanRun's output"""
    import torch
    from aad_amd.engine import ApiError
    groups = _golden_groups()
    checked = 0
    for key, recs in groups.items():
        images = [bf.case_of_record(r)["image"] for r in recs]
        # truncate every third image inside its last block (the plan's bytes-present rule)
        images = [img[:len(img) - 7] if i % 3 == 2 and _last_block_bytes(img, key[3]) > 18 * key[0] + 7 else img
                  for i, img in enumerate(images)]
        hd = parse_header(images[0][:31])
        flat, table = _pack(images)
        d_img = torch.from_numpy(flat).cuda()
        ch = hd.num_channels
        try:
            dplan = engine.decode_plan(hd, _with_pcm(table, ch), True)
        except ApiError as e:
            with pytest.raises(ApiError) as w:
                engine.window_decode_plan(hd, table, True)
            assert w.value.code == e.code, key
            continue
        total = int(table["num_samples"].astype(np.int64).sum())
        pcm = torch.zeros(total * ch + 16, dtype=torch.int16, device="cuda")
        dplan.run(d_img, pcm)
        host = pcm.cpu().numpy()
        dplan.close()
        offs = np.concatenate([[0], np.cumsum(table["num_samples"].astype(np.int64))])
        decoded = [host[offs[i] * ch:offs[i + 1] * ch].reshape(-1, ch) for i in range(len(images))]
        plan = engine.window_decode_plan(hd, table, True)
        lengths = [int(n) for n in table["num_samples"]]
        spb = hd.num_samples_per_block
        for frames in (1, 13, spb + 3, max(lengths)):
            _check(torch, plan, d_img, decoded, _windows_for(lengths, max(spb, 1), frames), frames, ch, ("golden", key))
        plan.close()
        checked += len(images)
    assert checked >= 800


def _last_block_bytes(img, block_size):
    payload = len(img) - 31
    return payload - (payload - 1) // block_size * block_size if payload > 0 else 0


def _with_pcm(table, ch):
    t = table.copy()
    t["pcm_offset"] = np.concatenate([[0], np.cumsum(t["num_samples"].astype(np.uint64))[:-1]]) * np.uint64(ch)
    return t


@pytest.mark.parametrize("ms", [False, True])
def test_segmented_encode_images(engine, ms):
    import torch
    pcm = torch.from_numpy(synth_pcm(6, 40000, 2, seed=77)).cuda()
    d_img, size = engine.encode_uniform(pcm, make_parameter(2, 4, 1024, 48000, ms, 0), segment_blocks=3, warmup_blocks=1)
    d_dec, _ = engine.decode_uniform(d_img, size)
    torch.cuda.synchronize()
    whole = d_dec.cpu().numpy()
    windows = torch.tensor([[0, 0], [5, 39000], [3, 12345], [2, 1], [6, 0]], dtype=torch.int64, device="cuda")
    for dtype in (torch.int16, torch.float32):
        got = engine.decode_windows(d_img, size, windows, 2000, dtype).cpu().numpy()
        want = window_expected(list(whole), windows.cpu().numpy(), 2000, 2, np.float32 if dtype == torch.float32 else np.int16)
        assert np.array_equal(got, want), dtype


def _corpus(engine, streams=16, samples=20000):
    import torch
    pcm = torch.from_numpy(synth_pcm(streams, samples, 2, seed=5)).cuda()
    d_img, size = engine.encode_uniform(pcm, make_parameter(2, 4, 1024))
    d_dec, hd = engine.decode_uniform(d_img, size)
    torch.cuda.synchronize()
    plan = engine.uniform_window_decode_plan(hd, streams, d_img.shape[1], size)
    return d_img, list(d_dec.cpu().numpy()), plan


def test_non_default_stream_and_randint_windows_without_sync(engine):
    import torch
    d_img, decoded, plan = _corpus(engine)
    side = torch.cuda.Stream()
    frames = 4800
    with torch.cuda.stream(side):
        src = d_img.clone()  # queued on the side stream: the run must be ordered behind it
        g = torch.Generator(device="cuda")
        g.manual_seed(3)
        windows = torch.stack([torch.randint(0, len(decoded), (256,), device="cuda", generator=g),
                               torch.randint(0, 20000 - frames, (256,), device="cuda", generator=g)], dim=1)
        torch.cuda.set_sync_debug_mode("error")  # any host synchronisation inside the run raises
        try:
            out = plan.run(src, windows, frames, torch.float32)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        done = torch.cuda.Event()
        done.record(side)
    done.synchronize()
    want = window_expected(decoded, windows.cpu().numpy(), frames, 2, np.float32)
    assert np.array_equal(out.cpu().numpy(), want)
    plan.close()


def test_signal_next_run_events(engine):
    import torch
    from aad_amd.engine import HipEvent
    d_img, decoded, plan = _corpus(engine)
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    windows = torch.tensor([[1, 100], [2, 3000], [15, 19000]], dtype=torch.int64, device="cuda")
    engine.signal_next(stop, start=start)
    out = plan.run(d_img, windows, 8000, torch.int16)
    stop.synchronize()
    assert start.elapsed_ms(stop) > 0
    assert np.array_equal(out.cpu().numpy(), window_expected(decoded, windows.cpu().numpy(), 8000, 2))
    plan.close()


def test_argument_errors(engine):
    import torch
    d_img, decoded, plan = _corpus(engine, streams=2, samples=3000)
    lib, h = engine.lib, plan.handle
    win = torch.tensor([[0, 0]], dtype=torch.int64, device="cuda")
    out = torch.zeros(2 * 100, dtype=torch.float32, device="cuda")
    run = lambda n, wp, frames, kind, op, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRun(h, data, n, wp, frames, kind, op)
    bad = AADApiResult.INVALID_ARGUMENT
    assert run(1, win.data_ptr(), 0, SAMPLE_INT16, out.data_ptr()) == bad                  # T = 0
    assert run(1, win.data_ptr(), 100, 2, out.data_ptr()) == bad                           # unknown sample type
    assert run(1, win.data_ptr(), 100, -1, out.data_ptr()) == bad
    assert run(1, None, 100, SAMPLE_FLOAT32, out.data_ptr()) == bad                        # null pointers with N > 0
    assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, None) == bad
    assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), data=None) == bad
    assert run(1 << 62, win.data_ptr(), 2, SAMPLE_INT16, out.data_ptr()) == bad            # N C T = 2^64 elements
    assert run((1 << 64) - 1, win.data_ptr(), 1, SAMPLE_INT16, out.data_ptr()) == bad
    assert lib.AADHip_WindowDecodePlanRun(None, None, 0, None, 1, 0, None) == bad
    assert run(0, None, 100, SAMPLE_INT16, None, data=None) == AADApiResult.OK             # nothing to do
    assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr()) == AADApiResult.OK
    torch.cuda.synchronize()
    assert np.array_equal(out[:200].cpu().numpy().reshape(1, 2, 100),
                          window_expected(decoded, [(0, 0)], 100, 2, np.float32))
    plan.close()
    # the plan validates like AADHip_DecodePlanCreate: same errors
    hd = parse_header(bytes(d_img[0, :31].cpu().numpy()))
    table = np.zeros(1, dtype=STREAM_DESC_DTYPE)
    table["data_size"], table["num_samples"] = 31 + 5, 3000  # a block shorter than its header
    for field, value in (("bits_per_sample", 5), ("num_channels", 9), (None, None)):
        h2 = parse_header(bytes(d_img[0, :31].cpu().numpy()))
        if field:
            setattr(h2, field, value)
        p1, p2 = C.c_void_p(), C.c_void_p()
        rc1 = lib.AADHip_DecodePlanCreate(engine._ctx, C.byref(h2), 1, 1, table.ctypes.data, C.byref(p1))
        rc2 = lib.AADHip_WindowDecodePlanCreate(engine._ctx, C.byref(h2), 1, 1, table.ctypes.data, C.byref(p2))
        assert rc1 == rc2 != AADApiResult.OK, field
    assert hd.num_channels == 2
