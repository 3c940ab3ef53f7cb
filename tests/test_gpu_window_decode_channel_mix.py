"""Channel-mix window decode on the device (AADHip_ChannelMixWindowDecodePlanCreate -> AADHip_WindowDecodePlanRun,
aad_amd/csrc/aad_decode_window_channel_mix.hip.h): crops of mono AND stereo streams, of any bits, block size and mid/side, into
planar [N, C, T] rows of one channel count - a mono stream into both rows of a stereo output, a stereo stream's mean into the one
row of a mono output, (L + R) >> 1 as int16 and (L + R) / 65536 as float32.

Bar: bit-exact against the definition (include/aad_hip.h; tests/channel_mix_oracle.py over each stream's OWN whole decode) -
  * a plan whose streams all have the output's channel count equals the mixed-format plan byte for byte;
  * a corpus interleaving mono and stereo streams of every (bits, block size, M/S) combination against the oracle's decodes, with
    every edge of the mixed test's window table, into a prefilled, guarded buffer; the stray windows under a stereo-source and
    under a mono-source first launch;
  * variants alternating window by window inside one wave (T = 1);
  * the corners of the sum (-65536, 65534, odd negative sums, a clipping M/S pair) from crafted channel headers;
  * truncated images against AADHip_DecodePlanRun of the same bytes, then the mix;
  * encode_planar of a mono and a stereo batch -> decode_windows_mixed(channels=...) against reconstruct_planar;
  * the constructor's errors, the run's errors and AADHip_ContextSignalNextRun's events on a many-kernel run."""
import ctypes as C
import struct

import numpy as np
import pytest

import bitstream_fuzz as bf
import oracle_binding as ob
from aad_amd.capi import AADApiResult, AADHeaderInfo, SAMPLE_FLOAT32, SAMPLE_INT16, STREAM_DESC_DTYPE, make_parameter
from aad_amd.engine import ApiError, parse_header
from aad_amd.synth import synth_pcm
from channel_mix_oracle import channel_mix_expected
from test_gpu_window_decode import _bare, _pack, _run
from test_gpu_window_decode_mixed import _compare, _decode_plan_rows, _edge_windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _check(torch, plan, d_img, decoded, windows, frames, out_channels, label):
    """int16 and float32 against the definition, both into a canary-filled buffer with guards (_run); float32 bitwise"""
    assert len(windows) <= 512 and frames <= 3000
    want = channel_mix_expected(decoded, windows, frames, out_channels, np.int16)
    _compare(_run(torch, plan, d_img, windows, frames, out_channels, torch.int16), want, label + ("int16",), windows)
    want32 = channel_mix_expected(decoded, windows, frames, out_channels, np.float32)
    got32 = _run(torch, plan, d_img, windows, frames, out_channels, torch.float32)
    _compare(got32.view(np.uint32), want32.view(np.uint32), label + ("float32 bits",), windows)


# ---- 1. streams that all have the output's channel count: the mixed-format plan's bytes ---------------------------------------
GEOMETRIES = [(c, b, False) for c in (1, 2) for b in (4, 3, 2)] + [(2, b, True) for b in (4, 3, 2)]


@pytest.mark.parametrize("with_header", [True, False], ids=["file", "bare"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dch%db%s" % (g[0], g[1], "ms" if g[2] else ""))
def test_same_channel_count_equals_the_mixed_format_plan(engine, geometry, with_header):
    import torch
    channels, bits, ms = geometry
    lengths = [2999, 777, 1, 1500]
    blocks = [256, 128, 256, 1024]  # the streams differ in block size: one variant, several geometries
    images = [ob.encode(synth_pcm(1, n, channels, seed=900 + 11 * i + channels * 31 + bits)[0], bits, mbs, 48000, ms, 0)
              for i, (n, mbs) in enumerate(zip(lengths, blocks))]
    headers = [parse_header(img[:31]) for img in images]
    spbs = [h.num_samples_per_block for h in headers]
    flat, table = _pack(images)
    if not with_header:
        table = _bare(table)
    d_img = torch.from_numpy(flat).cuda()
    mixed = engine.mixed_window_decode_plan(headers, table, with_header)
    mix = engine.channel_mix_window_decode_plan(headers, table, channels, with_header)
    try:
        for frames in (1, 16, min(spbs) - 1, min(spbs), min(spbs) + 2, 2999):
            windows = _edge_windows(lengths, spbs, frames)
            for dtype in (torch.int16, torch.float32):
                a = _run(torch, mixed, d_img, windows, frames, channels, dtype)
                b = _run(torch, mix, d_img, windows, frames, channels, dtype)
                assert a.tobytes() == b.tobytes(), (geometry, with_header, frames, dtype)
    finally:
        mixed.close()
        mix.close()


# ---- 2. a corpus of mono and stereo streams against the oracle ----------------------------------------------------------------
def _corpus():
    """every (bits, block size in 128 / 256 / 1024, M/S) stereo combination and every (bits, block size) mono one, two stereo
    streams then a mono one and so on, ragged lengths from 1 frame to 3000"""
    stereo = [(2, b, mbs, ms) for b in (4, 3, 2) for mbs in (128, 256, 1024) for ms in (False, True)]
    mono = [(1, b, mbs, False) for b in (4, 3, 2) for mbs in (128, 256, 1024)]
    rng = np.random.default_rng(77)
    stereo = [stereo[j] for j in rng.permutation(len(stereo))]
    mono = [mono[j] for j in rng.permutation(len(mono))]
    combos = []
    for i in range(9):
        combos += [stereo[2 * i], mono[i], stereo[2 * i + 1]]
    lengths = [1, 3000, 2, 5, 1] + [int(v) for v in rng.integers(6, 3000, size=len(combos) - 5)]
    for key in set((ch, bits, ms) for ch, bits, _, ms in combos):  # every variant has a stream of some length
        mine = [i for i, (ch, bits, _, ms) in enumerate(combos) if (ch, bits, ms) == key]
        if max(lengths[i] for i in mine) <= 300:
            lengths[mine[-1]] = 2500 - mine[-1]
    images, decoded = [], []
    for i, (ch, bits, mbs, ms) in enumerate(combos):
        img = ob.encode(synth_pcm(1, lengths[i], ch, seed=700 + 13 * i)[0], bits, mbs, 48000, ms, 0)
        images.append(img)
        decoded.append(ob.decode(img)[0])
    return images, decoded, lengths


def _variant(h):
    return (h.num_channels, h.bits_per_sample, int(h.num_channels == 2 and h.ch_process_method == 1))


@pytest.fixture(scope="module")
def corpus():
    """the reference, computed once: images, oracle decodes, lengths, headers, packed bytes, table"""
    images, decoded, lengths = _corpus()
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    return images, decoded, lengths, headers, flat, table


@pytest.mark.parametrize("with_header", [True, False], ids=["file", "bare"])
@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_corpus_equals_the_mix_of_each_streams_oracle_decode(engine, corpus, out_channels, with_header):
    import torch
    images, decoded, lengths, headers, flat, table = corpus
    assert len(images) == 27 and len({_variant(h) for h in headers}) == 9
    assert all(d.shape == (n, h.num_channels) for d, n, h in zip(decoded, lengths, headers))
    assert len({h.num_samples_per_block for h in headers}) >= 12
    spbs = [h.num_samples_per_block for h in headers]
    spb = min(spbs)
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table if with_header else _bare(table), out_channels, with_header)
    try:
        for frames in (1, 16, spb - 1, spb, spb + 2, 2999):  # 2999: every second int16 row at 2-byte alignment
            _check(torch, plan, d_img, decoded, _edge_windows(lengths, spbs, frames), frames, out_channels,
                   ("corpus", out_channels, with_header, frames))
    finally:
        plan.close()


@pytest.mark.parametrize("first", ["stereo_source_first", "mono_source_first"])
def test_stray_windows_under_either_first_launch(engine, corpus, first):
    """the run's first launch writes the windows whose stream is out of range, into out_channels rows each: with stereo streams in
    the plan that is a stereo-source launch (the six stereo variants come first), with mono streams alone a mono-source one"""
    import torch
    images, decoded, lengths, headers, _, _ = corpus
    keep = [i for i, h in enumerate(headers) if first == "stereo_source_first" or h.num_channels == 1]
    images, decoded, lengths, headers = ([v[i] for i in keep] for v in (images, decoded, lengths, headers))
    assert (headers[0].num_channels == 2 or all(h.num_channels == 1 for h in headers)) and len(images) >= 9
    assert any(h.num_channels == 2 for h in headers) == (first == "stereo_source_first")
    flat, table = _pack(images)
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    for out_channels in (2, 1):
        plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
        try:
            for frames in (1, min(spbs) + 2, 2999):
                windows = _edge_windows(lengths, spbs, frames)
                stray = [w for w, (s, _) in enumerate(windows.tolist()) if s % (1 << 64) >= len(images)]
                assert len(stray) >= 4  # the table makes the first launch write stray windows
                _check(torch, plan, d_img, decoded, windows, frames, out_channels, ("strays", first, out_channels, frames))
                # ... and alone, where no other launch writes anything
                _check(torch, plan, d_img, decoded, windows[stray], frames, out_channels, ("strays alone", first, out_channels, frames))
        finally:
            plan.close()


# ---- 3. variants inside one wave ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_variants_alternate_window_by_window_inside_a_wave(engine, corpus, out_channels):
    """T = 1: one lane per (window, source channel), so the lanes of a wave belong to mono, stereo L/R and stereo M/S windows in
    turn - the per-lane variant filter, the pair exchange next to lanes that do not exchange, and pairs at every lane parity a
    stereo launch gives them"""
    import torch
    images, decoded, lengths, headers, flat, table = corpus
    by_variant = {}
    for s, h in enumerate(headers):
        if lengths[s] > 300:
            by_variant.setdefault(_variant(h), s)
    order = sorted(by_variant, key=lambda v: (v[1], v[2], v[0]))  # mono, stereo L/R, stereo M/S, ... per bit width
    cycle = [by_variant[v] for v in order]
    assert len(cycle) == 9
    windows = np.array([(cycle[i % 9], (i * 37) % lengths[cycle[i % 9]]) for i in range(256)], dtype=np.int64)
    kinds = [_variant(headers[s]) for s in windows[:, 0]]
    assert all(a != b for a, b in zip(kinds, kinds[1:])) and {k[0] for k in kinds} == {1, 2} and {k[2] for k in kinds} == {0, 1}
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    try:
        _check(torch, plan, d_img, decoded, windows, 1, out_channels, ("wave", out_channels))
    finally:
        plan.close()


# ---- 4. corners of the sum ---------------------------------------------------------------------------------------------------
def _with_history(case, history):
    """the crafted image with every block's stored history samples replaced: history[c] = the four samples channel c's header
    emits first, in output order (the header holds them last first, behind the step word and between the weights)"""
    img = bytearray(case["image"])
    ch, bs = case["channels"], case["block_size"]
    for pos in range(bf.HEADER_BYTES, len(img), bs):
        for c in range(ch):
            for j, v in enumerate(history[c]):
                struct.pack_into(">h", img, pos + 18 * c + 4 + 4 * (3 - j), v)
    return bytes(img)


LR_HISTORY = [(-32768, 32767, -5, 100), (-32768, 32767, 2, -101)]  # sums -65536, 65534, -3, -1
MS_HISTORY = [(32767, -32768, 20000, -7), (32767, -32768, -20000, 4)]  # M + S = 65534 and -65536 clip on L; M - S = 40000 on R


def test_corners_of_the_sum_from_crafted_headers(engine):
    import torch
    images = []
    for bits in (4, 3, 2):
        for ms in (False, True):
            case = bf.make_case("mix-corner-%d-%d" % (bits, ms), channels=2, bits=bits, max_block_size=256, ms=ms, blocks=3,
                                body_kind="random", header_kind="encoderlike")
            assert case["num_samples"] > 2 * case["spb"]  # three blocks, each with headers of its own
            images.append(_with_history(case, MS_HISTORY if ms else LR_HISTORY))
    mono = bf.make_case("mix-corner-mono", channels=1, bits=4, max_block_size=256, blocks=2)
    images.append(_with_history(mono, [(-32768, 32767, -1, 1)]))
    headers = [parse_header(img[:31]) for img in images]
    decoded = [bf.oracle_decode(img) for img in images]
    # the corners are reached: asserted on the oracle's decode, before any comparison
    sums = set()
    for d, h in zip(decoded, headers):
        if h.num_channels == 2:
            s = d[:, 0].astype(np.int32) + d[:, 1].astype(np.int32)
            sums |= set(s.tolist())
            if h.ch_process_method == 0:
                assert s[:4].tolist() == [-65536, 65534, -3, -1]
                spb = h.num_samples_per_block
                assert s[spb:spb + 3].tolist() == [-65536, 65534, -3]  # ... in the second block too
            else:
                # L = clip16(M + S), R = clip16(M - S): both clip
                assert d[:4, 0].tolist() == [32767, -32768, 0, -3] and d[:4, 1].tolist() == [0, 0, 32767, -11]
                assert MS_HISTORY[0][0] + MS_HISTORY[1][0] > 32767 and MS_HISTORY[0][1] + MS_HISTORY[1][1] < -32768
                assert MS_HISTORY[0][2] - MS_HISTORY[1][2] > 32767
    assert {-65536, 65534, -3, -1} <= sums and any(s < 0 and s % 2 for s in sums)
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    for with_header in (False, True):  # bare blocks first: the crafted block headers are all there is
        for out_channels in (1, 2):
            plan = engine.channel_mix_window_decode_plan(headers, table if with_header else _bare(table), out_channels, with_header)
            try:
                for frames in (3, 4, 700):
                    windows = np.array([(s, f) for s in range(len(images)) for f in (0, 1, 2, spbs[s] - 1, spbs[s], spbs[s] + 1)],
                                       dtype=np.int64)
                    _check(torch, plan, d_img, decoded, windows, frames, out_channels, ("corners", with_header, out_channels, frames))
            finally:
                plan.close()


# ---- 5. truncated images -------------------------------------------------------------------------------------------------------
def test_truncated_images_decode_as_the_decode_plan_then_mix(engine, corpus):
    """cut just behind a block's channel headers, inside a wide chunk of an earlier block and inside the tail of the last block:
    each decodes as under AADHip_DecodePlanRun with the same data_size, and the mix is taken of that.  A cut INSIDE a channel header
    leaves a block shorter than its header: the plan is refused with AADHip_DecodePlanCreate's own error for that stream."""
    import torch
    images, _, lengths, headers, _, _ = corpus
    cut, kinds = [], {1: set(), 2: set()}
    for i, (img, h) in enumerate(zip(images, headers)):
        ch, bs = h.num_channels, h.block_size
        payload = len(img) - 31
        blocks = -(-payload // bs)
        last = payload - (blocks - 1) * bs
        kind, keep = "whole", len(img)
        if i % 4 == 0 and last > 18 * ch + 7:
            kind, keep = "tail", len(img) - 3                                   # the last units of the last block
        elif i % 4 == 1 and blocks > 1:
            kind, keep = "chunk", 31 + (blocks // 2) * bs + 18 * ch + (bs - 18 * ch) // 3  # inside an earlier block's codes
        elif i % 4 == 2:
            kind, keep = "headers", 31 + (blocks - 1) * bs + 18 * ch             # the last block: its channel headers alone
        elif blocks > 1:
            kind, keep = "chunk_start", 31 + (blocks - 1) * bs + 18 * ch + 5    # ... and a few code bytes: no wide load fits
        cut.append(img[:keep])
        kinds[ch].add(kind)
    assert all({"tail", "chunk", "headers"} <= kinds[ch] for ch in (1, 2)), kinds
    assert sum(len(a) != len(b) for a, b in zip(cut, images)) >= 16
    flat, table = _pack(cut)
    d_img = torch.from_numpy(flat).cuda()
    decoded = _decode_plan_rows(engine, torch, headers, table, d_img)  # AADHip_DecodePlanRun, one plan per format
    assert sum(not d[-1:].any() for d in decoded) >= 4                  # the cuts do lose samples
    spbs = [h.num_samples_per_block for h in headers]
    for out_channels in (1, 2):
        plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
        try:
            windows = np.array([(s, 0) for s in range(len(cut))] + [(s, max(lengths[s] - 300, 0)) for s in range(len(cut))], dtype=np.int64)
            _check(torch, plan, d_img, decoded, windows, 3000, out_channels, ("truncated", out_channels))
            _check(torch, plan, d_img, decoded, _edge_windows(lengths, spbs, 301), 301, out_channels, ("truncated edges", out_channels))
        finally:
            plan.close()
    # inside a channel header, a mono and a stereo stream
    for s in (next(i for i, h in enumerate(headers) if h.num_channels == c and lengths[i] > 5) for c in (1, 2)):
        short = table.copy()
        short["data_size"][s] = 31 + 18 * headers[s].num_channels - 5
        p1 = C.c_void_p()
        rc1 = engine.lib.AADHip_DecodePlanCreate(engine._ctx, C.byref(headers[s]), 1, 1, short[s:s + 1].ctypes.data, C.byref(p1))
        assert rc1 == AADApiResult.INSUFFICIENT_DATA
        assert _create(engine, 2, 1, len(cut), short, headers) == rc1 and _create(engine, 1, 1, len(cut), short, headers) == rc1


# ---- 6. Python level -----------------------------------------------------------------------------------------------------------
def test_encode_planar_of_mono_and_stereo_then_decode_windows_mixed(engine):
    import torch
    n, frames, length = 6, 700, 2500
    batches = []
    for ch, bits, ms in ((1, 3, False), (2, 4, True)):
        x = torch.from_numpy(np.ascontiguousarray(synth_pcm(n, length, ch, seed=51 + ch).transpose(0, 2, 1))).cuda()
        param = make_parameter(ch, bits, 256, 48000, ms, 0)
        images, sizes = engine.encode_planar(x, param)
        y = engine.reconstruct_planar(x, param, dtype=torch.int16)
        batches.append((images, [int(v) for v in sizes], y.cpu().numpy()))
    stride = max(int(b[0].shape[1]) for b in batches)
    data = torch.zeros((2 * n, stride), dtype=torch.uint8, device="cuda")
    sizes, decoded = [], []
    for k, (images, sz, y) in enumerate(batches):  # mono and stereo rows interleaved
        data[k::2, :images.shape[1]] = images
    for i in range(2 * n):
        sizes.append(batches[i % 2][1][i // 2])
        decoded.append(np.ascontiguousarray(batches[i % 2][2][i // 2].T))
    g = torch.Generator(device="cuda")
    g.manual_seed(19)
    windows = torch.stack([torch.randint(0, 2 * n, (256,), device="cuda", generator=g),
                           torch.randint(0, length - frames // 2, (256,), device="cuda", generator=g)], dim=1)
    host = windows.cpu().numpy()
    assert {int(s) % 2 for s in host[:, 0]} == {0, 1}
    for channels in (1, 2):
        got = engine.decode_windows_mixed(data, sizes, windows, frames, torch.int16, channels=channels).cpu().numpy()
        _compare(got, channel_mix_expected(decoded, host, frames, channels, np.int16), ("python", channels), host)
        got32 = engine.decode_windows_mixed(data, sizes, windows, frames, channels=channels).cpu().numpy()
        assert got32.dtype == np.float32 and got32.shape == (256, channels, frames)
        want32 = channel_mix_expected(decoded, host, frames, channels, np.float32)
        _compare(got32.view(np.uint32), want32.view(np.uint32), ("python float32", channels), host)
    with pytest.raises(ApiError):  # without the keyword the channel counts must agree, as before
        engine.decode_windows_mixed(data, sizes, windows, frames, torch.int16)
    with pytest.raises(ApiError):
        engine.decode_windows_mixed(data, sizes, windows, frames, torch.int16, channels=None)
    with pytest.raises(ApiError):
        engine.decode_windows_mixed(data, sizes, windows, frames, torch.int16, channels=3)


# ---- 7. errors and events ----------------------------------------------------------------------------------------------------
def _create(engine, out_channels, flag, n, table, formats, out=True):
    p = C.c_void_p()
    arr = (AADHeaderInfo * max(len(formats), 1))(*formats) if formats is not None else None
    rc = engine.lib.AADHip_ChannelMixWindowDecodePlanCreate(engine._ctx, out_channels, flag, n,
                                                            table.ctypes.data if table is not None else None,
                                                            C.addressof(arr) if arr is not None else None, C.byref(p) if out else None)
    if rc == AADApiResult.OK:
        engine.lib.AADHip_WindowDecodePlanDestroy(p)
    return rc


def test_error_matrix(engine, corpus):
    import torch
    images, decoded, lengths, headers, flat, table = corpus
    lib, bad = engine.lib, AADApiResult.INVALID_ARGUMENT
    n = len(images)
    copy = lambda h: AADHeaderInfo.from_buffer_copy(bytes(h))
    assert _create(engine, 2, 1, n, table, headers) == AADApiResult.OK and _create(engine, 1, 1, n, table, headers) == AADApiResult.OK
    # null arguments
    assert lib.AADHip_ChannelMixWindowDecodePlanCreate(None, 2, 1, n, table.ctypes.data, C.addressof((AADHeaderInfo * n)(*headers)),
                                                       C.byref(C.c_void_p())) == bad
    assert _create(engine, 2, 1, n, None, headers) == bad
    assert _create(engine, 2, 1, n, table, None) == bad
    assert _create(engine, 2, 1, n, table, headers, out=False) == bad
    assert _create(engine, 2, 1, 0, None, None) == AADApiResult.OK  # both may be null while num_streams == 0
    # the output's channel count, a stream's channel count
    assert _create(engine, 0, 1, n, table, headers) == bad
    assert _create(engine, 3, 1, n, table, headers) == bad
    for count in (3, 0, 8):
        wide = [copy(h) for h in headers]
        wide[5].num_channels = count
        assert _create(engine, 2, 1, n, table, wide) == bad and _create(engine, 1, 1, n, table, wide) == bad
    # one stream with an invalid format or table row: AADHip_DecodePlanCreate's code for it alone, the first failing stream's
    short = table.copy()
    short["data_size"][7] = 31 + 5  # a block shorter than its header
    seen = set()
    for field, value, tab in (("bits_per_sample", 5, table), ("bits_per_sample", 1, table), ("block_size", 18, table),
                              ("num_samples_per_block", 0, table), ("format_version", 99, table), (None, None, short)):
        broken = [copy(h) for h in headers]
        if field:
            setattr(broken[7], field, value)
        p1 = C.c_void_p()
        rc1 = lib.AADHip_DecodePlanCreate(engine._ctx, C.byref(broken[7]), 1, 1, tab[7:8].ctypes.data, C.byref(p1))
        assert rc1 not in (AADApiResult.OK, bad), (field, rc1)
        assert _create(engine, 2, 1, n, tab, broken) == rc1, field
        seen.add(rc1)
        later = [copy(h) for h in broken]
        later[20].num_channels = 5  # a later stream's channel count does not hide the earlier stream's error ...
        assert _create(engine, 1, 1, n, tab, later) == rc1, field
        later[3].num_channels = 5   # ... an earlier one's comes first
        assert _create(engine, 1, 1, n, tab, later) == bad, field
    assert len(seen) >= 2
    # M/S on a mono stream: as AADHip_DecodePlanCreate
    m1 = copy(next(h for h in headers if h.num_channels == 1))
    m1.ch_process_method = 1
    s1 = next(i for i, h in enumerate(headers) if h.num_channels == 1)
    p1 = C.c_void_p()
    rc1 = lib.AADHip_DecodePlanCreate(engine._ctx, C.byref(m1), 1, 1, table[s1:s1 + 1].ctypes.data, C.byref(p1))
    assert rc1 != AADApiResult.OK and _create(engine, 2, 1, 1, table[s1:s1 + 1], [m1]) == rc1
    # the run's errors are AADHip_WindowDecodePlanRun's, on N * out_channels * T elements
    d_img = torch.from_numpy(flat).cuda()
    win = torch.tensor([[1, 0]], dtype=torch.int64, device="cuda")
    out = torch.zeros(2 * 100, dtype=torch.float32, device="cuda")
    for out_channels in (1, 2):
        plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
        run = lambda k, wp, frames, kind, op, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRun(plan.handle, data, k, wp, frames, kind, op)
        assert run(1, win.data_ptr(), 0, SAMPLE_INT16, out.data_ptr()) == bad                  # T = 0
        assert run(1, win.data_ptr(), 100, 2, out.data_ptr()) == bad                           # unknown sample type
        assert run(1, win.data_ptr(), 100, -1, out.data_ptr()) == bad
        assert run(1, None, 100, SAMPLE_FLOAT32, out.data_ptr()) == bad                        # null pointers with N > 0
        assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, None) == bad
        assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), data=None) == bad
        assert run((1 << 62) // out_channels, win.data_ptr(), 1, SAMPLE_INT16, out.data_ptr()) == bad  # 2^64 float32 bytes
        assert run(0, None, 100, SAMPLE_INT16, None, data=None) == AADApiResult.OK             # num_windows == 0: nothing to do
        out.fill_(-7.0)
        assert run(0, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr()) == AADApiResult.OK  # ... launches nothing
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -7.0).all()
        assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr()) == AADApiResult.OK
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[:out_channels * 100].reshape(1, out_channels, 100),
                              channel_mix_expected(decoded, [(1, 0)], 100, out_channels, np.float32))
        plan.close()


@pytest.mark.parametrize("out_channels", [1, 2])
def test_no_streams_every_window_is_zero(engine, out_channels):
    import torch
    plan = engine.channel_mix_window_decode_plan([], np.zeros(0, dtype=STREAM_DESC_DTYPE), out_channels, True)
    data = torch.zeros(64, dtype=torch.uint8, device="cuda")
    windows = np.array([(0, 0), (5, 100), (-1, -1)], dtype=np.int64)
    for frames in (1, 300):
        for dtype in (torch.int16, torch.float32):
            assert not _run(torch, plan, data, windows, frames, out_channels, dtype).any()
    plan.close()


@pytest.mark.parametrize("out_channels", [1, 2])
def test_signal_next_run_events_on_a_nine_kernel_run(engine, corpus, out_channels):
    import torch
    from aad_amd.engine import HipEvent
    images, decoded, lengths, headers, flat, table = corpus  # nine variants: nine kernels
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    frames = 3000
    windows_np = np.array([(s, (7 * s) % lengths[s]) for s in range(len(images))] * 8, dtype=np.int64)
    windows = torch.from_numpy(windows_np).cuda()
    out = torch.full((len(windows_np), out_channels, frames), 0x5A5A, dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    engine.signal_next(stop, start=start)
    plan.run(d_img, windows, frames, torch.int16, out=out, ordered=False)  # torch's streams are not ordered behind the run ...
    stop.wait_on(side)                                                     # ... only the side stream, behind the stop event
    with torch.cuda.stream(side):
        snapshot = out.clone()
    side.synchronize()
    _compare(snapshot.cpu().numpy(), channel_mix_expected(decoded, windows_np, frames, out_channels), ("events",), windows_np)
    start.synchronize()
    stop.synchronize()
    assert start.elapsed_ms(stop) > 0
    plan.close()
