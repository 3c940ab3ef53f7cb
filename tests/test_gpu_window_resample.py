"""Window decode at another rate on the device (AADHip_ResamplerResolve -> AADHip_WindowDecodePlanRun -> AADHip_ResamplerRun,
aad_amd/csrc/aad_resample.hip): crops of a corpus resampled by a per-window rational ratio into planar [N, C, T] rows.

Bar: bit-exact against the definition (include/aad_hip.h "resample", restated in tests/resample_oracle.py with the library's own
banks, which tests/test_resample_host.py holds to the oracle's construction) over the int16 rows tests/window_oracle.py and
tests/channel_mix_oracle.py define -
  * a same-format corpus (streams of 700, 3000, 3000 and 40 frames, block size 256, 4-bit), a mixed-format one (4 / 3 / 2 bits)
    and a mono + stereo one into channels = 1 and channels = 2: the three kinds of window decode plan;
  * the ratios 1/1, 3/1, 1/3, 160/147, 147/160, 10/9, 10/11 and 160/441 in one run through `variant`, with 1024/1023 (a bank of
    53 KB) and 481/1340 (bank and span above 64 KB of LDS);
  * windows at frame 0, at 1, K/2 - 2, K/2 - 1 and K/2 (below, at and above the filter's lead), across the stream's end, at
    first_frame == num_samples and behind it, wrapped and huge values, a stream index past the table, -1, a variant past V, -1
    as a variant, a select entry of 0xFFFF;
  * T = 257 and T = 1025, one output past the FIR kernel's tile of 1024;
  * all four sample types, each into a buffer with canaries on both sides;
  * the (1, 1) ratio equal to Engine.decode_windows_mixed, byte for byte, for the four types;
  * Engine.decode_windows_resampled over headers of 16000, 44100 and 48000 Hz to 16000 Hz.  With speeds 9/10, 1 and 11/10 the
    44.1 kHz stream needs 16000 * 10 / (44100 * 9) = 1600/3969: L = 1600 is above the limit of 1024 phases and the call is
    refused, as AADHip_ResamplerCreate's limits say.  The rows are checked for all three rates at speed 1 and for the 16 kHz and
    48 kHz streams at the three speeds;
  * the C calls' refusals, which leave canaries untouched."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import resample_oracle as ro
from aad_amd.capi import AADApiResult, AADHipResampleRatio, ApiError, SAMPLE_FLOAT32, SAMPLE_INT16, STREAM_DESC_DTYPE
from aad_amd.engine import parse_header
from aad_amd.synth import synth_pcm
from channel_mix_oracle import mix_stream

pytestmark = pytest.mark.gpu

RATIOS = [(1, 1), (3, 1), (1, 3), (160, 147), (147, 160), (10, 9), (10, 11), (160, 441), (1024, 1023), (481, 1340)]
DTYPES = ("int16", "float32", "float16", "bfloat16")
FRAMES = (257, 1025)


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _rows(images):
    """images -> uint8 [S, pitch], STREAM_DESC_DTYPE table over the flattened tensor"""
    pitch = -(-max(len(i) for i in images) // 64) * 64 + 64
    data = np.zeros((len(images), pitch), dtype=np.uint8)
    table = np.zeros(len(images), dtype=STREAM_DESC_DTYPE)
    for i, img in enumerate(images):
        data[i, :len(img)] = np.frombuffer(img, dtype=np.uint8)
        table["data_offset"][i], table["data_size"][i] = i * pitch, len(img)
        table["num_samples"][i] = parse_header(img[:31]).num_samples
    return data, table


def _encode(lengths, channels, bits, rates=None, seed=900):
    images = []
    for i, n in enumerate(lengths):
        ch = channels[i] if isinstance(channels, (list, tuple)) else channels
        b = bits[i] if isinstance(bits, (list, tuple)) else bits
        pcm = synth_pcm(1, n, ch, seed=seed + 17 * i)[0]
        images.append(ob.encode(pcm, b, 256, rates[i] if rates else 48000, False, 0))
    return images


LENGTHS = [700, 3000, 3000, 40]


@pytest.fixture(scope="module")
def corpora():
    """name -> (images, data [S, pitch], table, headers, {channels: int16 rows per stream the plan of that kind decodes})"""
    out = {}
    for name, channels, bits in (("same", 2, 4), ("mixed", 1, [4, 3, 2, 4]), ("mix", [1, 2, 2, 1], [4, 3, 4, 2])):
        images = _encode(LENGTHS, channels, bits)
        decoded = [ob.decode(img)[0] for img in images]
        data, table = _rows(images)
        headers = [parse_header(img[:31]) for img in images]
        if name == "mix":
            rows = {c: [mix_stream(d, c) for d in decoded] for c in (1, 2)}
        else:
            rows = {channels: decoded}
        out[name] = (images, data, table, headers, rows)
    return out


def _banks(res):
    return [res.bank(r) for r in range(len(res.ratios))]


def _windows(banks, select):
    """windows and variants: per variant (bank) the edges of its own K, then the strays"""
    rows, variant = [], []
    for v, (L, M, h) in enumerate(banks):
        K = h.shape[1]
        s = 1 + v % 2  # the two streams of 3000 frames
        n = LENGTHS[s]
        firsts = [0, 1, max(K // 2 - 2, 0), K // 2 - 1, K // 2, 1234, n - 100, n - 1, n, n + K // 2 - 2, n + K]
        rows += [(s, f) for f in firsts] + [(0, 0), (0, 650), (3, 0), (3, 39), (3, 40)]
        variant += [v] * (len(firsts) + 5)
    V = len(banks)
    strays = [((len(LENGTHS), 5), 0), ((-1, 5), 0), (((1 << 63) - 1, 0), 1),      # no such stream
              ((1, 5), V), ((1, 5), -1), ((1, 5), 1 << 40),                     # no such variant
              ((1, -1), 1), ((2, 1 << 40), 2), ((2, -(1 << 62)), 3), ((1, (1 << 63) - 1), 4)]  # wrapped and huge starts
    rows += [s[0] for s in strays]
    variant += [s[1] for s in strays]
    none = [(s, v) for s in range(len(select)) for v in range(V) if select[s][v] == ro.NO_BANK]
    rows += [(s, 7) for s, v in none]
    variant += [v for s, v in none]
    return np.array(rows, dtype=np.int64), np.array(variant, dtype=np.int64)


def _bits(torch, t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint16)


def _run(torch, res, plan, d_img, windows, variant, frames, channels, name):
    """a run into a canary-bordered buffer -> the rows as the oracle's convert() gives them (int16, or the floats' bit patterns)"""
    dtype = getattr(torch, name)
    n = len(windows)
    count = n * channels * frames
    big = torch.full((count + 32,), 0x5A5A if name == "int16" else -7.0, dtype=dtype, device="cuda")
    out = big[16:16 + count].view(n, channels, frames)
    got = res.run(plan, d_img, torch.from_numpy(windows).cuda(), frames, variant=None if variant is None else torch.from_numpy(variant).cuda(),
                  dtype=dtype, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = _bits(torch, big)
    border = np.concatenate([host[:16], host[16 + count:]])
    assert (border == _bits(torch, torch.full((1,), 0x5A5A if name == "int16" else -7.0, dtype=dtype))[0]).all(), "wrote outside its rows"
    rows = host[16:16 + count].reshape(n, channels, frames)
    return rows.view(np.int16) if name == "int16" else rows


def _compare(got, want, label, windows, variant):
    if not np.array_equal(got, want):
        w, c, t = [int(v) for v in np.argwhere(got != want)[0]]
        raise AssertionError((label, "window", w, windows[w].tolist(), "variant", None if variant is None else int(variant[w]),
                              "channel", c, "t", t, got[w, c, t:t + 4].tolist(), want[w, c, t:t + 4].tolist()))


CASES = [("same", 2), ("mixed", 1), ("mix", 1), ("mix", 2)]


@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("case", CASES, ids=["same_format", "mixed_format", "channel_mix_mono", "channel_mix_stereo"])
def test_rows_equal_the_definition(engine, corpora, case, frames):
    import torch
    name, channels = case
    images, data, table, headers, rows = corpora[name]
    d_img = torch.from_numpy(data).cuda()
    if name == "same":
        plan = engine.window_decode_plan(headers[0], table)
    elif name == "mixed":
        plan = engine.mixed_window_decode_plan(headers, table)
    else:
        plan = engine.channel_mix_window_decode_plan(headers, table, channels)
    V = len(RATIOS)
    select = [[v for v in range(V)] for _ in LENGTHS]
    select[0][3] = select[2][0] = None  # 0xFFFF
    res = engine.resampler(RATIOS, select)
    try:
        banks = _banks(res)
        assert [(L, M) for L, M, _ in banks] == RATIOS and [h.shape[1] for _, _, h in banks] == [2, 24, 72, 24, 28, 24, 28, 68, 24, 68]
        assert res.source_frames(frames) == ro.source_frames(frames, [(L, M, h.shape[1]) for L, M, h in banks])
        table_select = [[ro.NO_BANK if v is None else v for v in row] for row in select]
        windows, variant = _windows(banks, table_select)
        acc = ro.expected_acc(rows[channels], windows, variant, table_select, banks, frames, channels)
        assert (acc != 0).any(axis=(1, 2)).sum() > len(windows) // 2
        for dtype in DTYPES:
            got = _run(torch, res, plan, d_img, windows, variant, frames, channels, dtype)
            _compare(got, ro.convert(acc, dtype), (case, frames, dtype), windows, variant)
        # no variant table: every window takes variant 0
        acc0 = ro.expected_acc(rows[channels], windows, None, table_select, banks, frames, channels)
        _compare(_run(torch, res, plan, d_img, windows, None, frames, channels, "int16"), ro.convert(acc0, "int16"),
                 (case, frames, "no variants"), windows, None)
    finally:
        res.close()
        plan.close()


def test_the_identity_ratio_equals_decode_windows_mixed(engine, corpora):
    import torch
    images, data, table, headers, rows = corpora["mixed"]
    d_img = torch.from_numpy(data).cuda()
    sizes = [len(i) for i in images]
    windows = np.array([(0, 0), (1, 5), (2, 2990), (3, 39), (3, 40), (1, 3000), (4, 0), (-1, 3), (2, -1), (0, 1 << 40)], dtype=np.int64)
    d_win = torch.from_numpy(windows).cuda()
    for frames in FRAMES:
        for name in DTYPES:
            dtype = getattr(torch, name)
            want = engine.decode_windows_mixed(d_img, sizes, d_win, frames, dtype)
            got = engine.decode_windows_resampled(d_img, sizes, d_win, frames, 48000, dtype=dtype)
            assert got.dtype == dtype and got.shape == want.shape
            assert _bits(torch, got).tobytes() == _bits(torch, want).tobytes(), (frames, name)


def test_decode_windows_resampled_reads_the_rates_from_the_headers(engine):
    import torch
    lengths, rates = [3000, 3000, 3000, 500], [16000, 44100, 48000, 48000]
    images = _encode(lengths, 2, [4, 3, 2, 4], rates=rates, seed=4100)
    decoded = [ob.decode(img)[0] for img in images]
    data, _ = _rows(images)
    d_img = torch.from_numpy(data).cuda()
    sizes = [len(i) for i in images]
    frames = 300
    windows = np.array([(s, f) for s in range(4) for f in (0, 7, 200, 2900)] + [(4, 0), (1, -1)], dtype=np.int64)

    def check(streams, speeds, variant):
        keep = [s for s in range(4) if s in streams]
        banks, select = [], []
        for s in keep:
            row = []
            for a, b in speeds:
                L, M = ro.reduce_ratio(16000 * b, rates[s] * a)
                if (L, M) not in [(x, y) for x, y, _ in banks]:
                    banks.append((L, M, ro.bank(L, M)))  # the oracle's own bank: within 1 of the library's per coefficient
                row.append([(x, y) for x, y, _ in banks].index((L, M)))
            select.append(row)
        rows_of = [decoded[s] for s in keep]
        win = windows.copy()
        local = {s: i for i, s in enumerate(keep)}
        win[:, 0] = [local.get(int(s), len(keep)) for s in win[:, 0]]
        d_rows = torch.from_numpy(np.ascontiguousarray(data[keep])).cuda()
        got = engine.decode_windows_resampled(d_rows, [sizes[s] for s in keep], torch.from_numpy(win).cuda(), frames, 16000, speeds=speeds,
                                              variant=None if variant is None else torch.from_numpy(variant).cuda(), dtype=torch.int16)
        # the library's banks for the same ratios, in the order decode_windows_resampled builds them
        res = engine.resampler([(L, M) for L, M, _ in banks], select)
        try:
            lib_banks = _banks(res)
        finally:
            res.close()
        for (L, M, h), (l2, m2, h2) in zip(banks, lib_banks):
            assert (L, M) == (l2, m2) and np.abs(h - h2).max() <= 1
        want = ro.expected(rows_of, win, variant, select, lib_banks, frames, 2, "int16")
        _compare(got.cpu().numpy(), want, (streams, speeds), win, variant)
        assert (want != 0).any()

    check((0, 1, 2, 3), ((1, 1),), None)  # 1/1, 160/441, 1/3
    variant = np.arange(len(windows), dtype=np.int64) % 3
    check((0, 2, 3), ((9, 10), (1, 1), (11, 10)), variant)  # 10/9, 1/1, 10/11 and 10/27, 1/3, 10/33
    # the 44.1 kHz stream at 9/10: 1600/3969, L above 1024 phases
    with pytest.raises(ApiError) as refused:
        engine.decode_windows_resampled(d_img, sizes, torch.from_numpy(windows).cuda(), frames, 16000, speeds=((9, 10), (1, 1), (11, 10)))
    assert refused.value.code == AADApiResult.INVALID_ARGUMENT


def test_refusals_write_nothing(engine, corpora):
    import torch
    lib, R = engine.lib, AADApiResult
    # creation
    handle = C.c_void_p(0x55)
    sel = (C.c_uint16 * 2)(0, 0xFFFF)
    ratio = lambda *pairs: (AADHipResampleRatio * len(pairs))(*[AADHipResampleRatio(u, d) for u, d in pairs])
    for pairs in ([(0, 1)], [(1, 0)], [(1025, 1)], [(1, 11)], [(1024, 1367)]):
        assert lib.AADHip_ResamplerCreate(engine._ctx, 1, ratio(*pairs), 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT, pairs
        assert handle.value is None
        handle = C.c_void_p(0x55)
    bad_sel = (C.c_uint16 * 2)(0, 1)
    assert lib.AADHip_ResamplerCreate(engine._ctx, 1, ratio((1, 1)), 1, 2, bad_sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert lib.AADHip_ResamplerCreate(engine._ctx, 1, ratio((1, 1)), 1, 0, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert lib.AADHip_ResamplerCreate(engine._ctx, 0, ratio((1, 1)), 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert lib.AADHip_ResamplerCreate(engine._ctx, 1, None, 1, 2, sel, C.byref(handle)) == R.INVALID_ARGUMENT
    assert lib.AADHip_ResamplerCreate(engine._ctx, 1, ratio((1, 1)), 1, 2, sel, None) == R.INVALID_ARGUMENT
    for pairs in ([(1024, 1)], [(3, 32)], [(1024, 1365)]):  # the largest accepted L, K and bank
        assert lib.AADHip_ResamplerCreate(engine._ctx, 1, ratio(*pairs), 1, 2, sel, C.byref(handle)) == R.OK, pairs
        lib.AADHip_ResamplerDestroy(handle)
    # runs
    res = engine.resampler([(1, 1), (3, 2)], [[0, 1]])
    try:
        n, ch, frames = 4, 2, 50
        t_src = res.source_frames(frames)
        assert t_src == 49 * 2 // 3 + 24
        L, M, K = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
        small = np.full(10, 77, dtype=np.int16)
        assert lib.AADHip_ResamplerBank(res.handle, 1, C.byref(L), C.byref(M), C.byref(K), small.ctypes.data, 10) == R.INSUFFICIENT_BUFFER
        assert lib.AADHip_ResamplerBank(res.handle, 2, C.byref(L), C.byref(M), C.byref(K), None, 0) == R.INVALID_ARGUMENT
        assert (L.value, M.value, K.value) == (9, 9, 9) and (small == 77).all()
        count = C.c_uint32(9)
        for bad_frames in (0, (1 << 31) // 2 + 2):  # (T - 1) * 2 >= 2^31
            assert lib.AADHip_ResamplerSourceFrames(res.handle, bad_frames, C.byref(count)) == R.INVALID_ARGUMENT and count.value == 9
        windows = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        src_windows = torch.full((n, 2), 0x5A5A, dtype=torch.int64, device="cuda")
        lanes = torch.full((n, 2), 0x5A5A, dtype=torch.int32, device="cuda")
        src = torch.full((n, ch, t_src), 0x5A5A, dtype=torch.int16, device="cuda")
        out = torch.full((n, ch, frames), -7.0, dtype=torch.float32, device="cuda")
        w, sw, ln, sp, op = (t.data_ptr() for t in (windows, src_windows, lanes, src, out))
        resolve = lib.AADHip_ResamplerResolve
        assert resolve(None, n, w, None, frames, sw, ln) == R.INVALID_ARGUMENT
        assert resolve(res.handle, n, None, None, frames, sw, ln) == R.INVALID_ARGUMENT
        assert resolve(res.handle, n, w, None, frames, None, ln) == R.INVALID_ARGUMENT
        assert resolve(res.handle, n, w, None, frames, sw, None) == R.INVALID_ARGUMENT
        assert resolve(res.handle, n, w, None, 0, sw, ln) == R.INVALID_ARGUMENT
        assert resolve(res.handle, n, w + 4, None, frames, sw, ln) == R.INVALID_ARGUMENT
        assert resolve(res.handle, n, w, w + 4, frames, sw, ln) == R.INVALID_ARGUMENT
        assert resolve(res.handle, n, w, None, frames, sw, ln + 2) == R.INVALID_ARGUMENT
        assert resolve(res.handle, 0, w, None, frames, sw, ln) == R.OK  # no window: no launch
        run = lib.AADHip_ResamplerRun
        f32 = SAMPLE_FLOAT32
        assert run(None, n, ch, sp, t_src, ln, frames, f32, op) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, None, t_src, ln, frames, f32, op) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, sp, t_src, None, frames, f32, op) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, sp, t_src, ln, frames, f32, None) == R.INVALID_ARGUMENT
        assert run(res.handle, n, 0, sp, t_src, ln, frames, f32, op) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, sp, t_src, ln, 0, f32, op) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, sp, t_src - 1, ln, frames, f32, op) == R.INVALID_ARGUMENT  # source rows too short
        for kind in (2, 3, 6, -1):
            assert run(res.handle, n, ch, sp, t_src, ln, frames, kind, op) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, sp + 1, t_src, ln, frames, f32, op) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, sp, t_src, ln, frames, f32, op + 2) == R.INVALID_ARGUMENT
        assert run(res.handle, n, ch, sp, t_src, ln, frames, SAMPLE_INT16, op + 1) == R.INVALID_ARGUMENT
        assert run(res.handle, 1 << 62, ch, sp, t_src, ln, frames, f32, op) == R.INVALID_ARGUMENT  # N * C * T past 64 bits
        many = (1 << 64) // (2 * t_src) // ch + 10 ** 14  # N * C * T * 2 fits 64 bits, N * C * T_src * 2 does not
        assert many * ch * frames * 2 < 1 << 64 <= many * ch * t_src * 2
        assert run(res.handle, many, ch, sp, t_src, ln, frames, SAMPLE_INT16, op) == R.INVALID_ARGUMENT
        assert run(res.handle, 0, ch, sp, t_src, ln, frames, f32, op) == R.OK
        engine.synchronize()
        assert (src_windows.cpu().numpy() == 0x5A5A).all() and (lanes.cpu().numpy() == 0x5A5A).all()
        assert (out.cpu().numpy() == -7.0).all()
        assert "resampler" in engine.last_error()
    finally:
        res.close()
