"""The spectrogram stage on the device (AADHip_SpectrogramRun, aad_amd/csrc/aad_spectrogram.hip): int16 rows into power spectra
or filterbank energies, the sums as int8 matrix products.

Bar: bit for bit against the definition (include/aad_hip.h "spectrogram", restated in tests/spectrogram_oracle.py), canaries on
both sides of every output.  The inputs are tests/spectrogram_matrix.py's, on which tests/test_spectrogram_host.py shows that
each of eight mistakes a kernel could make changes an output of a case here.
  * small, every edge: hand-made rows (noise, all -32768, alternating rails, silence), n_fft 96, W 80, B 49 - two k-steps, the
    second with 16 taps, four column tile pairs, the last with one bin - H in {16, 37, 80, 96}, T such that F is one more than the
    kernel's frame tile (read from the header through the driver), the rows at pitch T + 0, 1 and 37 with rails behind T and at
    both pointer parities, once with M = 0 and once with the five awkward filters;
  * shapes: W 64 and 65 at n_fft 128; W = n_fft = 16 with H = 1; n_fft 512, W 400, H 160 with 80 mel filters over four rows of
    T = 4000; n_fft = W = 4096 over one rail row of two frames with sums next to 2^42;
  * the item loop: 2^20 + 77 rows of one frame, a sample on the host and every row against a closed form on the device;
  * two runs over a pre-filled `out`; the C call's refusals and num_rows == 0;
  * Engine.mel_windows over a mixed corpus; Convolver.run(dtype=torch.int16) -> Spectrogram.run against both oracles composed."""
import ctypes as C
import time

import numpy as np
import pytest

import convolve_oracle as co
import spectrogram_matrix as sm
import spectrogram_oracle as so
from aad_amd.capi import AADApiResult
from test_gpu_window_resample import corpora, engine  # noqa: F401

pytestmark = pytest.mark.gpu

CANARY = 0xC0E00000  # -7.0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sm.build_driver(tmp_path_factory.mktemp("spectrogram"))


class Out:
    """a float32 device buffer of `shape` with 16 canaries on both sides"""

    def __init__(self, torch, shape, fill=CANARY):
        self.torch, self.shape, self.count = torch, tuple(shape), int(np.prod(shape))
        bits = np.full(self.count + 32, CANARY, dtype=np.uint32)
        bits[16:16 + self.count] = fill
        self.big = torch.from_numpy(bits.view(np.int32)).cuda().view(torch.float32)
        self.view = self.big[16:16 + self.count].view(*self.shape)

    def bits(self):
        host = self.big.view(self.torch.int32).cpu().numpy().view(np.uint32)
        assert (host[:16] == CANARY).all() and (host[16 + self.count:] == CANARY).all(), "wrote outside its buffer"
        return host[16:16 + self.count].reshape(self.shape)


def _same(got_bits, want, label):
    want_bits = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert got_bits.shape == want_bits.shape, (label, got_bits.shape, want_bits.shape)
    bad = np.argwhere(got_bits != want_bits)
    assert bad.size == 0, "%s: %d of %d elements differ, the first at %s: got %08x, want %08x" % (
        label, len(bad), got_bits.size, tuple(bad[0]), got_bits[tuple(bad[0])], want_bits[tuple(bad[0])])


def _device_rows(torch, rows, extra=0, parity=0):
    """the rows on the device as a [R, T] view of pitch T + extra that starts `parity` elements into its buffer"""
    buf, offset, pitch = sm.strided(rows, extra, parity)
    d = torch.from_numpy(buf).cuda()
    return d, torch.as_strided(d, rows.shape, (pitch, 1), offset)


@pytest.mark.parametrize("H", sm.SMALL_HOPS)
def test_small_every_edge(engine, driver, H):  # noqa: F811
    import torch
    started = time.time()
    pitch, tile_frames, frame_major, _, _ = sm.geometry(driver, sm.SMALL_W, H)
    assert bool(frame_major) == (H % 16 != 0) and pitch == (128 if frame_major else H)
    T = sm.small_frames(H, tile_frames)
    rows, window = sm.hand_made_rows(T), so.hann(sm.SMALL_W)
    B = so.bins(sm.SMALL_FFT)
    for filters in (None, sm.awkward_filters(B)):
        want = so.spectrogram_rows(rows, window, sm.SMALL_FFT, H, filters)
        assert want.shape == (4, tile_frames + 1, B if filters is None else 5)
        assert not want[3].view(np.uint32).any() and want[:3].any()  # silence: every output +0
        if filters is not None:
            assert not want[:, :, 0].view(np.uint32).any()  # the all-zero filter
        spec = engine.spectrogram(sm.SMALL_FFT, H, sm.SMALL_W, window, filters)
        try:
            assert spec.frames(T) == tile_frames + 1
            q, m = spec.coefficients()
            oq, cq, sq = so.quantise(window, sm.SMALL_FFT)
            assert q == oq and np.array_equal(m[:, :, 0], cq) and np.array_equal(m[:, :, 1], sq)
            for extra in (0, 1, 37):
                for parity in (0, 1):
                    keep, view = _device_rows(torch, rows, extra, parity)
                    assert view.data_ptr() % 4 == 2 * parity
                    out = Out(torch, want.shape)
                    assert spec.run(view, out=out.view).data_ptr() == out.view.data_ptr()
                    _same(out.bits(), want, ("H", H, "filters", filters is not None, "pitch", T + extra, "parity", parity))
        finally:
            spec.close()
    print("small H=%d: %.2f s" % (H, time.time() - started))


@pytest.mark.parametrize("name", list(sm.SHAPES))
def test_shapes(engine, name):  # noqa: F811
    import torch
    started = time.time()
    s = sm.SHAPES[name]
    rows, window, filters = sm.shape_inputs(name)
    want = so.spectrogram_rows(rows, window, s.n_fft, s.H, filters)
    spec = engine.spectrogram(s.n_fft, s.H, s.W, window, filters)
    try:
        out = Out(torch, want.shape)
        spec.run(torch.from_numpy(rows).cuda(), out=out.view)
        _same(out.bits(), want, name)
        if name == "common":  # [N, C, T] rows give [N, C, F, M], and window=None is the periodic Hann window
            default = engine.spectrogram(s.n_fft, s.H, s.W, None, filters)
            try:
                got = default.run(torch.from_numpy(rows).cuda().view(2, 2, s.T))
                assert got.shape == (2, 2) + want.shape[1:]
                _same(got.view(torch.int32).cpu().numpy().view(np.uint32).reshape(want.shape), want, "common, [N, C, T]")
            finally:
                default.close()
    finally:
        spec.close()
    print("shape %s: %.2f s" % (name, time.time() - started))


def test_the_limit_two_frames_of_4096_with_sums_next_to_2_42(engine):  # noqa: F811
    import torch
    started = time.time()
    row, window, q, cq, sq = sm.limit_inputs()
    Re, Im = so.sums(row[0], cq, sq, sm.LIMIT_H)
    assert q == 14 and Re.shape == (2, 2049) and abs(int(Re[0, 5])) > 0.6 * 2 ** 42
    want = so.power(Re, Im, q)[None]
    spec = engine.spectrogram(sm.LIMIT_FFT, sm.LIMIT_H, window=window)
    try:
        out = Out(torch, want.shape)
        spec.run(torch.from_numpy(row).cuda(), out=out.view)
        _same(out.bits(), want, "limit")
    finally:
        spec.close()
    print("limit: %.2f s" % (time.time() - started))


def test_the_item_loop_past_2_20_workgroups(engine):  # noqa: F811
    """row r is zero but for element r % 16, which holds a(r): Re[k] = a cq[r % 16][k], Im[k] = a sq[r % 16][k]"""
    import torch
    started = time.time()
    R, n = (1 << 20) + 77, 16
    window = so.hann(n)
    q, cq, sq = so.quantise(window, n)
    r = torch.arange(R, device="cuda", dtype=torch.int64)
    a = (r * 7919) % 65536 - 32768
    rows = torch.zeros((R, n), dtype=torch.int16, device="cuda")
    rows[r, r % n] = a.to(torch.int16)
    spec = engine.spectrogram(n, 1, window=window)
    try:
        out = Out(torch, (R, 1, so.bins(n)))
        spec.run(rows, out=out.view)
        # every row against the closed form, on the device: int64 -> float32 rounds to nearest even, each float32 operation a kernel
        scale = torch.tensor(2.0 ** -(15 + q), dtype=torch.float32, device="cuda")
        re = (a[:, None] * torch.from_numpy(cq.astype(np.int64)).cuda()[r % n]).to(torch.float32) * scale
        im = (a[:, None] * torch.from_numpy(sq.astype(np.int64)).cuda()[r % n]).to(torch.float32) * scale
        rr = re * re
        ii = im * im
        want = rr + ii
        assert torch.equal(out.view[:, 0, :].view(torch.int32), want.view(torch.int32))
        got = out.bits()
        host_rows = rows.cpu().numpy()
        for i in [0, 1, 15, 16, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, R - 1] + list(range(12345, R, 99991)):
            _same(got[i], so.spectrogram(host_rows[i], window, n, 1), ("row", i))
    finally:
        spec.close()
    print("item loop: %.2f s" % (time.time() - started))


def test_two_runs_over_a_prefilled_out_give_the_same_bits(engine):  # noqa: F811
    import torch
    rows, window, filters = sm.shape_inputs("common")
    s = sm.SHAPES["common"]
    spec = engine.spectrogram(s.n_fft, s.H, s.W, window, filters)
    try:
        d_rows = torch.from_numpy(rows).cuda()
        F = spec.frames(s.T)
        first, second = Out(torch, (s.rows, F, s.mels), 0x7FC01234), Out(torch, (s.rows, F, s.mels), 0x3F800000)
        spec.run(d_rows, out=first.view)
        spec.run(d_rows, out=second.view)
        spec.run(d_rows, out=second.view)  # over its own result: no element is accumulated into
        assert np.array_equal(first.bits(), second.bits())
        _same(first.bits(), so.spectrogram_rows(rows, window, s.n_fft, s.H, filters), "prefilled")
    finally:
        spec.close()


def test_the_c_calls_refusals_and_the_empty_run(engine):  # noqa: F811
    import torch
    lib, bad = engine.lib, AADApiResult.INVALID_ARGUMENT
    window = so.hann(80)
    filters = sm.awkward_filters(49)
    handle = C.c_void_p()

    def create(n_fft, W, H, win, M, f):
        h = C.c_void_p()
        rc = lib.AADHip_SpectrogramCreate(engine._ctx, n_fft, W, H, None if win is None else win.ctypes.data, M,
                                          None if f is None else f.ctypes.data, C.byref(h))
        assert (rc == AADApiResult.OK) == bool(h.value)
        if h.value:
            lib.AADHip_SpectrogramDestroy(h)
        return rc
    assert create(96, 80, 16, window, 5, filters) == AADApiResult.OK
    assert create(96, 0, 16, window, 0, None) == bad and create(64, 80, 16, window, 0, None) == bad
    assert create(8192, 80, 16, window, 0, None) == bad and create(96, 80, 0, window, 0, None) == bad
    assert create(96, 80, 16, None, 0, None) == bad
    assert create(96, 80, 16, window, 5, None) == bad and create(96, 80, 16, window, 0, filters) == bad
    spoiled = window.copy()
    spoiled[3] = np.nan
    assert create(96, 80, 16, spoiled, 0, None) == bad and create(96, 80, 16, window * np.float32(40000), 0, None) == bad
    for value in (np.inf, 2.0 ** -61):
        f = filters.copy()
        f[2, 7] = value
        assert create(96, 80, 16, window, 5, f) == bad
    assert lib.AADHip_SpectrogramCreate(engine._ctx, 96, 80, 16, window.ctypes.data, 0, None, C.byref(handle)) == AADApiResult.OK
    try:
        T = 80 + 16 * 3
        rows = torch.zeros(2 * T + 8, dtype=torch.int16, device="cuda")
        out = Out(torch, (2, 4, 49))
        p, o = rows.data_ptr(), out.view.data_ptr()
        n = C.c_uint32(7)
        assert lib.AADHip_SpectrogramFrames(handle, 79, C.byref(n)) == bad and n.value == 7
        assert lib.AADHip_SpectrogramFrames(handle, T, C.byref(n)) == AADApiResult.OK and n.value == 4
        for refused in ((2, None, T, T, o), (2, p, T, T, None), (2, p + 1, T, T, o), (2, p, T, T, o + 2), (2, p, T, 79, o),
                        (2, p, T - 1, T, o), (1 << 63, p, T, T, o), (1 << 62, p, T, T, o)):
            assert lib.AADHip_SpectrogramRun(handle, *refused) == bad, refused
        assert lib.AADHip_SpectrogramRun(None, 2, p, T, T, o) == bad
        assert lib.AADHip_SpectrogramRun(handle, 0, p, T, T, o) == AADApiResult.OK  # launches nothing
        torch.cuda.synchronize()
        assert (out.bits() == CANARY).all()  # a refused call writes nothing
        assert lib.AADHip_SpectrogramRun(handle, 2, p, T, T, o) == AADApiResult.OK
        torch.cuda.synchronize()
        assert not out.bits().any()  # silence
    finally:
        lib.AADHip_SpectrogramDestroy(handle)


def _window_rows(decoded, windows, frames, channels):
    """int16 [N, channels, frames]: the crops of the decoded streams, zeros where a stream has no frame"""
    out = np.zeros((len(windows), channels, frames), dtype=np.int16)
    for w, (s, f) in enumerate(windows.tolist()):
        d = decoded[s]
        n = max(0, min(frames, len(d) - f))
        out[w, :, :n] = d[f:f + n].T
    return out


def test_mel_windows_over_a_mixed_corpus(engine, corpora):  # noqa: F811
    import torch
    from aad_amd.engine import mel_filters
    images, data, table, headers, rows = corpora["mix"]
    d_img = torch.from_numpy(data).cuda()
    sizes = [len(i) for i in images]
    windows = np.array([(0, 0), (1, 5), (2, 2500), (3, 0), (1, 1234), (0, 300)], dtype=np.int64)
    frames, n_fft, W, H = 600, 256, 200, 80
    filters = mel_filters(16000, n_fft, 23)
    assert np.allclose(filters, so.mel_filters(16000, n_fft, 23), rtol=2.0 ** -22, atol=0)
    for channels in (1, 2):
        want = so.spectrogram_rows(_window_rows(rows[channels], windows, frames, channels), so.hann(W), n_fft, H, filters)
        got = engine.mel_windows(d_img, sizes, torch.from_numpy(windows).cuda(), frames, n_fft, H, filters, channels=channels, win_length=W)
        assert got.shape == (len(windows), channels, 1 + (frames - W) // H, 23) and got.is_contiguous()
        _same(got.view(torch.int32).cpu().numpy().view(np.uint32), want, ("mel_windows", channels))


def test_convolver_int16_rows_through_the_spectrogram(engine, corpora):  # noqa: F811
    import torch
    images, data, table, headers, rows = corpora["mixed"]
    d_img = torch.from_numpy(data).cuda()
    rng = np.random.default_rng(3)
    hs = [(rng.uniform(-0.5, 0.5, size=K) * np.exp(-np.arange(K) * (5.0 / K))).astype(np.float32) for K in (17, 200)]
    for h in hs:
        h[2] = 1.0
    windows = np.array([(1, 100), (2, 250), (1, 2900), (0, 10)], dtype=np.int64)
    index = np.array([0, 1, 1, 0], dtype=np.int64)
    frames, n_fft, H = 700, 128, 32
    plan = engine.mixed_window_decode_plan(headers, table)
    conv = engine.convolver(hs)
    spec = engine.spectrogram(n_fft, H)
    try:
        responses = []
        for h in hs:
            taps, q, delay = co.quantise(h, None)
            responses.append((taps.astype(np.int64), q, delay))
        wet = np.zeros((len(windows), 1, frames), dtype=np.int16)
        for w, (s, f) in enumerate(windows.tolist()):
            acc = co.row(rows[1][s][:, 0], len(rows[1][s]), f, frames, responses[index[w]])
            wet[w, 0] = co.element_bits(acc, responses[index[w]][1], "int16").view(np.int16)
        d_wet = conv.run(plan, d_img, torch.from_numpy(windows).cuda(), frames, response=torch.from_numpy(index).cuda(), dtype=torch.int16)
        assert np.array_equal(d_wet.cpu().numpy(), wet)
        got = spec.run(d_wet)
        _same(got.view(torch.int32).cpu().numpy().view(np.uint32), so.spectrogram_rows(wet, so.hann(n_fft), n_fft, H), "convolver chain")
    finally:
        spec.close()
        conv.close()
        plan.close()
