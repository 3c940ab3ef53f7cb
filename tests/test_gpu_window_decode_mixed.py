"""Mixed-format window decode on the device (AADHip_MixedWindowDecodePlanCreate -> AADHip_WindowDecodePlanRun,
aad_amd/csrc/aad_decode_window_mixed.hip.h): crops of streams that do not share bits, block size or mid/side into planar
[N, C, T] rows, one kernel per (bits, mid/side) variant of the plan.

Bar: bit-exact against the definition (include/aad_hip.h; tests/window_oracle.py over each stream's OWN whole decode) -
  * a plan whose streams share a format equals the same-format plan byte for byte;
  * a corpus of every (bits, block size, M/S) combination against the oracle's decodes, with every edge of the same-format test's
    window table, into a prefilled, guarded buffer;
  * variants alternating window by window inside one wave (T = 1);
  * the crafted images of tests/golden/bitstream_fuzz.json and truncated images against AADHip_DecodePlanRun;
  * encode_planar_mixed -> decode_windows_mixed against encode_planar / reconstruct_planar;
  * the constructor's errors, the run's errors and AADHip_ContextSignalNextRun's events on a three-kernel run."""
import ctypes as C

import numpy as np
import pytest

import bitstream_fuzz as bf
import oracle_binding as ob
from aad_amd.capi import AADApiResult, AADHeaderInfo, SAMPLE_FLOAT32, SAMPLE_INT16, STREAM_DESC_DTYPE, make_parameter
from aad_amd.engine import parse_header
from aad_amd.synth import synth_pcm
from test_gpu_window_decode import _bare, _pack, _run, _with_pcm
from window_oracle import window_expected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _key(h):
    return (h.num_channels, h.bits_per_sample, h.block_size, h.num_samples_per_block, h.ch_process_method)


def _edge_windows(lengths, spbs, frames):
    """every edge of the same-format test's table, per stream with that stream's own block length"""
    rows = []
    for s, (n, spb) in enumerate(zip(lengths, spbs)):
        rows += [(s, 0), (s, spb - 1), (s, spb), (s, (n * 3) // 7), (s, max(n - frames, 0)), (s, max(n - frames // 2 - 1, 0)),
                 (s, n - 1), (s, n)]
    rows += [(0, lengths[0] + 5), (1, 1 << 40), (2, -1), (3, -(1 << 62)),             # past the end, huge, wrapped
             (len(lengths), 0), ((1 << 63) - 1, 7), (-1, 0), (len(lengths) + 1, 5)]  # stream out of range
    return np.array(rows, dtype=np.int64)


def _compare(got, want, label, windows):
    if not np.array_equal(got, want):
        w, c, t = [int(v) for v in np.argwhere(got != want)[0]]
        raise AssertionError((label, "window", w, windows[w].tolist(), "channel", c, "t", t, got[w, c, t:t + 4].tolist(),
                              want[w, c, t:t + 4].tolist()))


def _check(torch, plan, d_img, decoded, windows, frames, channels, label):
    """int16 against the definition, float32 = int16 / 32768 bitwise; both into a canary-filled buffer with guards (_run)"""
    assert len(windows) <= 512 and frames <= 3000
    want = window_expected(decoded, windows, frames, channels)
    _compare(_run(torch, plan, d_img, windows, frames, channels, torch.int16), want, label, windows)
    got32 = _run(torch, plan, d_img, windows, frames, channels, torch.float32)
    want32 = want.astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(got32.view(np.uint32), want32.view(np.uint32)), (label, frames, "float32 is not int16 / 32768")


# ---- 1. one-variant plans equal the existing plan ----------------------------------------------------------------------------
GEOMETRIES = [(c, b, False) for c in (1, 2, 3, 8) for b in (4, 3, 2)] + [(2, b, True) for b in (4, 3, 2)]


@pytest.mark.parametrize("with_header", [True, False], ids=["file", "bare"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dch%db%s" % (g[0], g[1], "ms" if g[2] else ""))
def test_one_variant_plan_equals_the_same_format_plan(engine, geometry, with_header):
    import torch
    channels, bits, ms = geometry
    lengths = [2999, 777, 1, 1500]
    images = [ob.encode(synth_pcm(1, n, channels, seed=300 + 11 * i + channels * 31 + bits)[0], bits, 256, 48000, ms, 0)
              for i, n in enumerate(lengths)]
    hd = parse_header(images[0][:31])
    spb = hd.num_samples_per_block
    flat, table = _pack(images)
    if not with_header:
        table = _bare(table)
    d_img = torch.from_numpy(flat).cuda()
    same = engine.window_decode_plan(hd, table, with_header)
    mixed = engine.mixed_window_decode_plan([parse_header(img[:31]) for img in images], table, with_header)
    try:
        for frames in (1, 16, spb - 1, spb, spb + 2, 3000):
            windows = _edge_windows(lengths, [spb] * len(lengths), frames)
            for dtype in (torch.int16, torch.float32):
                a = _run(torch, same, d_img, windows, frames, channels, dtype)
                b = _run(torch, mixed, d_img, windows, frames, channels, dtype)
                assert a.tobytes() == b.tobytes(), (geometry, with_header, frames, dtype)
    finally:
        same.close()
        mixed.close()


# ---- 2. a mixed corpus against the oracle ------------------------------------------------------------------------------------
def _corpus(channels):
    """every (bits, block size in 128 / 256 / 1024, M/S for stereo) combination, ragged lengths from 1 frame to 3000"""
    combos = [(b, mbs, ms) for b in (4, 3, 2) for mbs in (128, 256, 1024) for ms in ((False, True) if channels == 2 else (False,))]
    combos += combos[:6] if channels == 2 else combos[:3]
    rng = np.random.default_rng(2024 + channels)
    lengths = [1, 3000, 2, 5] + [int(v) for v in rng.integers(6, 3000, size=len(combos) - 4)]
    order = rng.permutation(len(combos))  # variants interleaved stream by stream
    images, decoded = [], []
    for i, j in enumerate(order):
        bits, mbs, ms = combos[j]
        img = ob.encode(synth_pcm(1, lengths[i], channels, seed=500 + 13 * i + channels)[0], bits, mbs, 48000, ms, 0)
        images.append(img)
        decoded.append(ob.decode(img)[0])
    return images, decoded, lengths


@pytest.fixture(scope="module")
def corpora():
    """the reference, computed once: channels -> (images, oracle decodes, lengths, headers, packed bytes, table)"""
    out = {}
    for channels in (1, 2):
        images, decoded, lengths = _corpus(channels)
        headers = [parse_header(img[:31]) for img in images]
        flat, table = _pack(images)
        out[channels] = (images, decoded, lengths, headers, flat, table)
    return out


@pytest.mark.parametrize("with_header", [True, False], ids=["file", "bare"])
@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
def test_mixed_corpus_equals_slices_of_each_streams_oracle_decode(engine, corpora, channels, with_header):
    import torch
    images, decoded, lengths, headers, flat, table = corpora[channels]
    assert len(images) == (24 if channels == 2 else 12)
    assert len({(h.bits_per_sample, h.ch_process_method) for h in headers}) == (6 if channels == 2 else 3)
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table if with_header else _bare(table), with_header)
    try:
        for frames in (1, 7, min(spbs), min(spbs) + 2, 3000):
            _check(torch, plan, d_img, decoded, _edge_windows(lengths, spbs, frames), frames, channels, ("corpus", channels, frames))
    finally:
        plan.close()


# ---- 3. variants inside one wave ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo_ms_next_to_lr"])
def test_variants_alternate_window_by_window_inside_a_wave(engine, corpora, channels):
    """T = 1: one lane per (window, channel), so the lanes of a wave belong to every variant in turn - the per-lane variant filter
    and (stereo) the pair exchange between an M/S window's two lanes, next to L/R windows that do not exchange"""
    import torch
    images, decoded, lengths, headers, flat, table = corpora[channels]
    by_variant = {}
    for s, h in enumerate(headers):
        if lengths[s] > 300:
            by_variant.setdefault((h.bits_per_sample, h.ch_process_method), s)
    cycle = [by_variant[k] for k in sorted(by_variant)]
    assert len(cycle) == (6 if channels == 2 else 3)
    windows = np.array([(cycle[i % len(cycle)], (i * 37) % lengths[cycle[i % len(cycle)]]) for i in range(256)], dtype=np.int64)
    if channels == 2:
        kinds = [headers[s].ch_process_method for s in windows[:, 0]]
        assert any(a != b for a, b in zip(kinds, kinds[1:]))  # an M/S window next to an L/R one
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)
    try:
        _check(torch, plan, d_img, decoded, windows, 1, channels, ("wave", channels))
    finally:
        plan.close()


# ---- 4. / 5. crafted and truncated images against AADHip_DecodePlanRun -------------------------------------------------------
def _decode_plan_rows(engine, torch, headers, table, d_img):
    """what AADHip_DecodePlanRun writes per stream (into zeros), one decode plan per format"""
    groups = {}
    for i, h in enumerate(headers):
        groups.setdefault(_key(h), []).append(i)
    decoded = [None] * len(headers)
    for idx in groups.values():
        ch = headers[idx[0]].num_channels
        sub = _with_pcm(table[idx], ch)
        dplan = engine.decode_plan(headers[idx[0]], sub, True)
        total = int(sub["num_samples"].astype(np.int64).sum())
        pcm = torch.zeros(total * ch + 16, dtype=torch.int16, device="cuda")
        dplan.run(d_img, pcm)
        host = pcm.cpu().numpy()
        dplan.close()
        offs = np.concatenate([[0], np.cumsum(sub["num_samples"].astype(np.int64))])
        for j, i in enumerate(idx):
            decoded[i] = host[offs[j] * ch:offs[j + 1] * ch].reshape(-1, ch)
    return decoded


def _whole_stream_rows(engine, torch, images, channels, label):
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    d_img = torch.from_numpy(flat).cuda()
    decoded = _decode_plan_rows(engine, torch, headers, table, d_img)
    frames = max(int(n) for n in table["num_samples"])
    windows = np.array([(s, 0) for s in range(len(images))], dtype=np.int64)
    plan = engine.mixed_window_decode_plan(headers, table, True)
    try:
        want = window_expected(decoded, windows, frames, channels)  # each row: the stream transposed, then a zero tail
        got = _run(torch, plan, d_img, windows, frames, channels, torch.int16)
        _compare(got, want, label, windows)
    finally:
        plan.close()
    return headers


@pytest.mark.parametrize("channels", [1, 2])
def test_crafted_bitstreams_in_one_plan(engine, channels):
    """all the golden crafted images of a channel count in ONE plan (random headers and bodies, ragged and truncated images, the
    inconsistent-geometry family: many block sizes, many samples_per_block, below 4 too)"""
    import torch
    images = [bf.case_of_record(r)["image"] for r in bf.golden_cases() if r["channels"] == channels]
    assert len(images) >= 200
    headers = _whole_stream_rows(engine, torch, images, channels, ("golden", channels))
    assert min(h.num_samples_per_block for h in headers) < 4
    assert len({(h.bits_per_sample, h.ch_process_method) for h in headers}) == (6 if channels == 2 else 3)
    assert len({h.block_size for h in headers}) > 20


def test_truncated_images_of_different_formats(engine, corpora):
    """cut inside the last block, inside an earlier block and just behind a block's channel headers: each decodes as under
    AADHip_DecodePlanRun with the same data_size"""
    import torch
    images, _, lengths, headers, _, _ = corpora[2]
    cut = []
    for i, (img, h) in enumerate(zip(images, headers)):
        payload, bs = len(img) - 31, h.block_size
        blocks = -(-payload // bs)
        if i % 4 == 0:
            keep = len(img) - 7 if payload - (blocks - 1) * bs > 36 + 7 else len(img)
        elif i % 4 == 1 and blocks > 1:
            keep = 31 + (blocks // 2) * bs + 36 + (bs - 36) // 3  # inside an earlier block
        elif i % 4 == 2:
            keep = 31 + (blocks - 1) * bs + 36                     # the last block: its channel headers alone
        else:
            keep = len(img)
        cut.append(img[:keep])
    assert sum(len(a) != len(b) for a, b in zip(cut, images)) >= 12
    _whole_stream_rows(engine, torch, cut, 2, ("truncated",))


# ---- 6. producer and consumer ------------------------------------------------------------------------------------------------
def test_encode_planar_mixed_then_decode_windows_mixed(engine):
    import torch
    n, frames = 12, 700
    x = torch.from_numpy(np.ascontiguousarray(synth_pcm(n, 2500, 2, seed=41).transpose(0, 2, 1))).cuda()
    bits = torch.tensor([2, 3, 4] * 4, dtype=torch.int64, device="cuda")
    make = lambda b: make_parameter(2, b, 256, 48000, b == 3, 0)
    images, sizes = engine.encode_planar_mixed(x, make, bits)
    host = images.cpu().numpy()
    rows = {}
    for b in (2, 3, 4):
        y, img_b, sizes_b = engine.reconstruct_planar(x, make(b), dtype=torch.int16, return_images=True)
        alone, sizes_alone = engine.encode_planar(x, make(b))
        assert np.array_equal(alone.cpu().numpy(), img_b.cpu().numpy()) and sizes_alone == sizes_b
        rows[b] = (y.cpu().numpy(), alone.cpu().numpy(), sizes_b)
    for i in range(n):
        b = int(bits[i])
        assert sizes[i] == rows[b][2][i]
        assert host[i, :sizes[i]].tobytes() == rows[b][1][i, :sizes[i]].tobytes(), i
        assert not host[i, sizes[i]:].any()
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    windows = torch.stack([torch.randint(0, n, (256,), device="cuda", generator=g),
                           torch.randint(0, 2500 - frames // 2, (256,), device="cuda", generator=g)], dim=1)
    got = engine.decode_windows_mixed(images, sizes, windows, frames, torch.int16).cpu().numpy()
    decoded = [rows[int(bits[i])][0][i].T for i in range(n)]
    want = window_expected(decoded, windows.cpu().numpy(), frames, 2)
    _compare(got, want, ("producer",), windows.cpu().numpy())
    got32 = engine.decode_windows_mixed(images, sizes, windows, frames).cpu().numpy()
    assert np.array_equal(got32.view(np.uint32), (want.astype(np.float32) / np.float32(32768.0)).view(np.uint32))


# ---- 7. errors and events ----------------------------------------------------------------------------------------------------
def _create(engine, channels, flag, n, table, formats, out=True):
    p = C.c_void_p()
    arr = (AADHeaderInfo * max(len(formats), 1))(*formats) if formats is not None else None
    rc = engine.lib.AADHip_MixedWindowDecodePlanCreate(engine._ctx, channels, flag, n, table.ctypes.data if table is not None else None,
                                                       C.addressof(arr) if arr is not None else None, C.byref(p) if out else None)
    if rc == AADApiResult.OK:
        engine.lib.AADHip_WindowDecodePlanDestroy(p)
    return rc


def test_error_matrix(engine, corpora):
    import torch
    images, decoded, lengths, headers, flat, table = corpora[2]
    lib, bad = engine.lib, AADApiResult.INVALID_ARGUMENT
    n = len(images)
    copy = lambda h: AADHeaderInfo.from_buffer_copy(bytes(h))
    assert _create(engine, 2, 1, n, table, headers) == AADApiResult.OK
    # null arguments
    assert lib.AADHip_MixedWindowDecodePlanCreate(None, 2, 1, n, table.ctypes.data, C.addressof((AADHeaderInfo * n)(*headers)),
                                                  C.byref(C.c_void_p())) == bad
    assert _create(engine, 2, 1, n, None, headers) == bad
    assert _create(engine, 2, 1, n, table, None) == bad
    assert _create(engine, 2, 1, n, table, headers, out=False) == bad
    # the channel count
    assert _create(engine, 0, 1, n, table, headers) == bad
    assert _create(engine, 9, 1, n, table, headers) == bad
    mono = [copy(h) for h in headers]
    mono[5].num_channels = 1
    mono[5].ch_process_method = 0
    assert _create(engine, 2, 1, n, table, mono) == bad
    # one stream with an invalid format or table row: AADHip_DecodePlanCreate's code for it alone
    short = table.copy()
    short["data_size"][7] = 31 + 5  # a block shorter than its header
    for field, value, tab in (("bits_per_sample", 5, table), ("bits_per_sample", 1, table), ("block_size", 36, table),
                              ("num_samples_per_block", 0, table), ("format_version", 99, table), (None, None, short)):
        broken = [copy(h) for h in headers]
        if field:
            setattr(broken[7], field, value)
        p1 = C.c_void_p()
        rc1 = lib.AADHip_DecodePlanCreate(engine._ctx, C.byref(broken[7]), 1, 1, tab[7:8].ctypes.data, C.byref(p1))
        assert rc1 not in (AADApiResult.OK, bad), (field, rc1)
        assert _create(engine, 2, 1, n, tab, broken) == rc1, field
    # M/S on a channel count other than two: as AADHip_DecodePlanCreate
    m3 = AADHeaderInfo.from_buffer_copy(bytes(headers[0]))
    m3.num_channels, m3.ch_process_method = 3, 1
    p1 = C.c_void_p()
    rc1 = lib.AADHip_DecodePlanCreate(engine._ctx, C.byref(m3), 1, 1, table[:1].ctypes.data, C.byref(p1))
    assert rc1 != AADApiResult.OK and _create(engine, 3, 1, 1, table[:1], [m3]) == rc1
    # the run's errors are AADHip_WindowDecodePlanRun's
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)
    win = torch.tensor([[0, 0]], dtype=torch.int64, device="cuda")
    out = torch.zeros(2 * 100, dtype=torch.float32, device="cuda")
    run = lambda k, wp, frames, kind, op, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRun(plan.handle, data, k, wp, frames, kind, op)
    assert run(1, win.data_ptr(), 0, SAMPLE_INT16, out.data_ptr()) == bad                  # T = 0
    assert run(1, win.data_ptr(), 100, 2, out.data_ptr()) == bad                           # unknown sample type
    assert run(1, win.data_ptr(), 100, -1, out.data_ptr()) == bad
    assert run(1, None, 100, SAMPLE_FLOAT32, out.data_ptr()) == bad                        # null pointers with N > 0
    assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, None) == bad
    assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), data=None) == bad
    assert run(1 << 62, win.data_ptr(), 2, SAMPLE_INT16, out.data_ptr()) == bad            # N C T = 2^64 elements
    assert run(0, None, 100, SAMPLE_INT16, None, data=None) == AADApiResult.OK             # num_windows == 0: nothing to do
    assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr()) == AADApiResult.OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(1, 2, 100), window_expected(decoded, [(0, 0)], 100, 2, np.float32))
    plan.close()


def test_no_streams_every_window_is_zero(engine):
    import torch
    plan = engine.mixed_window_decode_plan([], np.zeros(0, dtype=STREAM_DESC_DTYPE), True, num_channels=2)
    data = torch.zeros(64, dtype=torch.uint8, device="cuda")
    windows = np.array([(0, 0), (5, 100), (-1, -1)], dtype=np.int64)
    for frames in (1, 300):
        for dtype in (torch.int16, torch.float32):
            assert not _run(torch, plan, data, windows, frames, 2, dtype).any()
    plan.close()


def test_signal_next_run_events_on_a_three_kernel_run(engine, corpora):
    import torch
    from aad_amd.engine import HipEvent
    images, decoded, lengths, headers, flat, table = corpora[1]  # mono: three variants, three kernels
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)
    frames = 3000
    windows_np = np.array([(s, (7 * s) % lengths[s]) for s in range(len(images))] * 8, dtype=np.int64)
    windows = torch.from_numpy(windows_np).cuda()
    out = torch.full((len(windows_np), 1, frames), 0x5A5A, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    engine.signal_next(stop, start=start)
    plan.run(d_img, windows, frames, torch.int16, out=out, ordered=False)  # torch's streams are not ordered behind the run ...
    stop.wait_on(side)                                                     # ... only the side stream, behind the stop event
    with torch.cuda.stream(side):
        snapshot = out.clone()
    side.synchronize()
    _compare(snapshot.cpu().numpy(), window_expected(decoded, windows_np, frames, 1), ("events",), windows_np)
    start.synchronize()
    stop.synchronize()
    assert start.elapsed_ms(stop) > 0
    plan.close()
