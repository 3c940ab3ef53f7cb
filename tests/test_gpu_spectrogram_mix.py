"""The mix of the spectrogram stage on the device (AADHip_SpectrogramRunMix, aad_amd/csrc/aad_spectrogram_mix.hip): two int16 row
batches summed at gains and quantised while the kernel stages them, then the stage's sums on the matrix cores.

Bar: bit for bit against the definition (include/aad_hip.h "spectrogram", paragraph "mix", restated in
tests/spectrogram_mix_oracle.py followed by tests/spectrogram_oracle.py), canaries on both sides of every output.  The inputs are
tests/spectrogram_mix_matrix.py's, on which tests/test_spectrogram_mix_host.py shows that each of nine mistakes a kernel could make
changes an output bit of a case here, and counts the witnesses.
  * small, every edge: n_fft 96, W 80, H in {16, 37} - one per staging mode - T such that F is one more than the frame tile, four
    rows as two groups; a the hand-made rows, b noise with the planted fused-multiply-add witnesses, +32767, rails in phase, noise;
    gains NULL, halves (ties) and signed (both rails clip); spans NULL, (T, 0), an odd span at an odd offset across the tile boundary beside an empty
    one through o >= T with L = 2^64 - 1, and an L past the row beside L = 0; a at pitch T + 1 and b at T + 37 at pointer parities
    (1, 0) and (0, 1) with rails behind every row; once with M = 0 and once with the awkward filters;
  * identity: gb = 0 over rails, and Le = 0, give the bits of Spectrogram.run(a);
  * NaN and infinite gains; the item loop past 2^20 workgroups with a gain per group of three rows; two runs over a pre-filled
    `out`; the C call's refusals, one per rule, and the empty run;
  * Engine.mel_mix_windows over the small corpora, with and without noise_spans: against the oracle over the numpy mix of the two
    int16 decodes, and - without a down-mix - against Spectrogram.run of clamp(rint(32768 mix_windows(float32)))."""
import ctypes as C
import time

import numpy as np
import pytest

import spectrogram_matrix as sm
import spectrogram_mix_matrix as mm
import spectrogram_mix_oracle as mo
import spectrogram_oracle as so
from aad_amd.capi import AADApiResult
from test_gpu_spectrogram import CANARY, Out, _device_rows, _same, _window_rows
from test_gpu_window_resample import corpora, engine  # noqa: F401

pytestmark = pytest.mark.gpu


def _gain(torch, g):
    return None if g is None else torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()


def _spans(torch, spans):
    return None if spans is None else torch.from_numpy(mm.span_table(spans)).cuda()


def _bits(torch, t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("H", mm.SMALL_HOPS)
def test_small_every_edge(engine, H):  # noqa: F811
    import torch
    started = time.time()
    T, a, b, cases = mm.small_cases(H)
    window = so.hann(sm.SMALL_W)
    B = so.bins(sm.SMALL_FFT)
    views = []
    for parity in mm.PARITIES:
        keep_a, view_a = _device_rows(torch, a, mm.PITCH_EXTRA[0], parity[0])
        keep_b, view_b = _device_rows(torch, b, mm.PITCH_EXTRA[1], parity[1])
        assert (view_a.data_ptr() % 4, view_b.data_ptr() % 4) == (2 * parity[0], 2 * parity[1])
        assert (view_a.stride(0), view_b.stride(0)) == (T + 1, T + 37)
        views.append((keep_a, keep_b, view_a, view_b))
    mixes = [(label, ga, gb, spans, mo.mix_rows(a, b, mm.ROWS_PER_GAIN, ga, gb, spans)) for label, ga, gb, spans in cases]
    assert any((x == 32767).any() and (x == -32768).any() for *_, x in mixes)
    for filters in (None, sm.awkward_filters(B)):
        spec = engine.spectrogram(sm.SMALL_FFT, H, sm.SMALL_W, window, filters)
        try:
            assert spec.frames(T) == mm.SMALL_TILE_FRAMES + 1
            for label, ga, gb, spans, x in mixes:
                want = mo.spectrogram_mix_rows(x, window, sm.SMALL_FFT, H, filters).reshape(2, 2, mm.SMALL_TILE_FRAMES + 1, -1)
                for _, _, view_a, view_b in views:
                    out = Out(torch, want.shape)
                    # [N, C, T] views of pitched rows: rows_per_gain = C = 2, one gain pair and one span per window
                    rows = torch.as_strided(view_a, (2, 2, T), (2 * view_a.stride(0), view_a.stride(0), 1))
                    other = torch.as_strided(view_b, (2, 2, T), (2 * view_b.stride(0), view_b.stride(0), 1))
                    got = spec.run_mix(rows, other, _gain(torch, ga), _gain(torch, gb), _spans(torch, spans), out=out.view)
                    assert got.data_ptr() == out.view.data_ptr()
                    _same(out.bits(), want, ("H", H, "filters", filters is not None, label, "a at", view_a.data_ptr() % 4))
        finally:
            spec.close()
    print("small mix H=%d: %.2f s" % (H, time.time() - started))


def test_identity_with_the_plain_run(engine):  # noqa: F811
    import torch
    H = 37
    T, a, b = mm.small_rows(H)
    rails = np.where(np.arange(4 * T).reshape(4, T) % 2 == 0, 32767, -32768).astype(np.int16)
    spec = engine.spectrogram(sm.SMALL_FFT, H, sm.SMALL_W, so.hann(sm.SMALL_W), sm.awkward_filters(so.bins(sm.SMALL_FFT)))
    try:
        d_a, d_rails = torch.from_numpy(a).cuda(), torch.from_numpy(rails).cuda()
        plain = Out(torch, (4, mm.SMALL_TILE_FRAMES + 1, 5))
        spec.run(d_a, out=plain.view)
        zero = Out(torch, plain.shape)
        spec.run_mix(d_a, d_rails, other_gain=torch.zeros(4, device="cuda"), out=zero.view)
        assert np.array_equal(zero.bits(), plain.bits())
        empty = Out(torch, plain.shape)
        spec.run_mix(d_a, d_rails, other_gain=torch.full((4,), 3.0, device="cuda"),
                     spans=_spans(torch, [(5, T), (2 ** 64 - 1, T + 1), (0, 0), (7, 2 ** 63)]), out=empty.view)
        assert np.array_equal(empty.bits(), plain.bits())
        same = Out(torch, plain.shape)  # a and b the same memory: 0.5 a + 0.5 a
        spec.run_mix(d_a, d_a, torch.full((4,), 0.5, device="cuda"), torch.full((4,), 0.5, device="cuda"), out=same.view)
        assert np.array_equal(same.bits(), plain.bits())
    finally:
        spec.close()


def test_nan_and_infinite_gains(engine):  # noqa: F811
    import torch
    a, b, ga, gb = mm.special_gain_case()
    x = mo.mix_rows(a, b, 1, ga, gb, None)
    assert not x[0].any() and (x[2, [0, 1, 2]] != 0).all() and x[2, 7] == 0 and x[4, 11] == 0  # a NaN m gives 0, an infinite one the rail
    assert set(np.unique(x[3])) <= {-32768, 0, 32767} and (np.abs(x[5].astype(np.int32)) >= 32767).sum() >= a.shape[1] - 2
    window = so.hann(sm.SMALL_W)
    want = mo.spectrogram_mix_rows(x, window, sm.SMALL_FFT, 16)
    spec = engine.spectrogram(sm.SMALL_FFT, 16, sm.SMALL_W, window)
    try:
        out = Out(torch, want.shape)
        spec.run_mix(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), _gain(torch, ga), _gain(torch, gb), out=out.view)
        _same(out.bits(), want, "special gains")
    finally:
        spec.close()


def test_the_item_loop_past_2_20_workgroups(engine):  # noqa: F811
    """rows a and b are zero but for element r % 16, which holds a(r) and b(r): the staged row holds x(r) there, and
    Re[k] = x cq[r % 16][k], Im[k] = x sq[r % 16][k]; a gain pair per group of three rows"""
    import torch
    started = time.time()
    R, n, per = (1 << 20) + 77, 16, 3
    assert R % per == 0
    window = so.hann(n)
    q, cq, sq = so.quantise(window, n)
    r = torch.arange(R, device="cuda", dtype=torch.int64)
    a = (r * 7919) % 65536 - 32768
    b = (r * 104729) % 65536 - 32768
    G = torch.arange(R // per, device="cuda", dtype=torch.int64)
    ga = (((G * 31) % 97).to(torch.float32) / 64.0 - 0.7).contiguous()
    gb = (((G * 17) % 89).to(torch.float32) / 48.0 - 0.9).contiguous()
    rows_a = torch.zeros((R, n), dtype=torch.int16, device="cuda")
    rows_b = torch.zeros((R, n), dtype=torch.int16, device="cuda")
    rows_a[r, r % n] = a.to(torch.int16)
    rows_b[r, r % n] = b.to(torch.int16)
    spec = engine.spectrogram(n, 1, window=window)
    try:
        out = Out(torch, (R, 1, so.bins(n)))
        spec.run_mix(rows_a.view(R // per, per, n), rows_b.view(R // per, per, n), ga, gb, out=out.view.view(R // per, per, 1, so.bins(n)))
        # every row against the closed form, on the device: each float32 operation a kernel of its own, torch.round ties to even
        pa = ga[r // per] * a.to(torch.float32)
        pb = gb[r // per] * b.to(torch.float32)
        x = torch.round(pa + pb).clamp(-32768, 32767).to(torch.int64)
        scale = torch.tensor(2.0 ** -(15 + q), dtype=torch.float32, device="cuda")
        re = (x[:, None] * torch.from_numpy(cq.astype(np.int64)).cuda()[r % n]).to(torch.float32) * scale
        im = (x[:, None] * torch.from_numpy(sq.astype(np.int64)).cuda()[r % n]).to(torch.float32) * scale
        rr = re * re
        ii = im * im
        want = rr + ii
        assert torch.equal(out.view[:, 0, :].view(torch.int32), want.view(torch.int32))
        got = out.bits()
        h_ga, h_gb = ga.cpu().numpy(), gb.cpu().numpy()
        for i in [0, 1, 2, 3, 15, 16, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, R - 1] + list(range(12345, R, 99991)):
            xi = mo.mix_rows(rows_a[i:i + 1].cpu().numpy(), rows_b[i:i + 1].cpu().numpy(), 1, h_ga[i // per: i // per + 1], h_gb[i // per: i // per + 1])
            assert xi[0, i % n] == int(x[i]) and np.count_nonzero(xi) <= 1
            _same(got[i], so.spectrogram(xi[0], window, n, 1), ("row", i))
    finally:
        spec.close()
    print("mix item loop: %.2f s" % (time.time() - started))


def test_two_runs_over_a_prefilled_out_give_the_same_bits(engine):  # noqa: F811
    import torch
    rows, window, filters = sm.shape_inputs("common")
    s = sm.SHAPES["common"]
    other = np.random.default_rng(41).integers(-32768, 32768, size=rows.shape).astype(np.int16)
    ga, gb = np.array([1.0, 0.8], dtype=np.float32), np.array([0.31, -0.6], dtype=np.float32)
    spans = [(1500, 777), (s.T, 0)]
    spec = engine.spectrogram(s.n_fft, s.H, s.W, window, filters)
    try:
        d_rows, d_other = torch.from_numpy(rows).cuda().view(2, 2, s.T), torch.from_numpy(other).cuda().view(2, 2, s.T)
        F = spec.frames(s.T)
        first, second = Out(torch, (2, 2, F, s.mels), 0x7FC01234), Out(torch, (2, 2, F, s.mels), 0x3F800000)
        args = (d_rows, d_other, _gain(torch, ga), _gain(torch, gb), _spans(torch, spans))
        spec.run_mix(*args, out=first.view)
        spec.run_mix(*args, out=second.view)
        spec.run_mix(*args, out=second.view)  # over its own result: no element is accumulated into
        assert np.array_equal(first.bits(), second.bits())
        x = mo.mix_rows(rows, other, 2, ga, gb, spans)
        _same(first.bits().reshape(4, F, s.mels), mo.spectrogram_mix_rows(x, window, s.n_fft, s.H, filters), "prefilled mix")
    finally:
        spec.close()


def test_the_c_calls_refusals_and_the_empty_run(engine):  # noqa: F811
    import torch
    lib, bad = engine.lib, AADApiResult.INVALID_ARGUMENT
    window = so.hann(80)
    handle = C.c_void_p()
    assert lib.AADHip_SpectrogramCreate(engine._ctx, 96, 80, 16, window.ctypes.data, 0, None, C.byref(handle)) == AADApiResult.OK
    try:
        T = 80 + 16 * 3
        rows = torch.zeros(5 * T, dtype=torch.int16, device="cuda")
        other = torch.zeros(5 * T, dtype=torch.int16, device="cuda")
        gains = torch.ones(8, dtype=torch.float32, device="cuda")
        spans = torch.tensor([[T, 0]] * 5, dtype=torch.int64, device="cuda")
        out = Out(torch, (4, 4, 49))
        a, b, g, s, o = rows.data_ptr(), other.data_ptr(), gains.data_ptr(), spans.data_ptr(), out.view.data_ptr()
        good = dict(n=4, a=a, pa=T, b=b, pb=T + 2, per=2, ga=g, gb=g + 4, sp=s, T=T, o=o)
        run = lambda **change: lib.AADHip_SpectrogramRunMix(handle, *dict(good, **change).values())
        for refused in (dict(a=None), dict(b=None), dict(o=None), dict(a=a + 1), dict(b=b + 1), dict(o=o + 2), dict(T=79), dict(pa=T - 1),
                        dict(pb=T - 1), dict(n=1 << 63), dict(n=1 << 62), dict(per=0), dict(per=3), dict(ga=g + 2), dict(gb=g + 1),
                        dict(sp=s + 4)):
            assert run(**refused) == bad, refused
        assert lib.AADHip_SpectrogramRunMix(None, *good.values()) == bad
        assert run(n=0) == AADApiResult.OK and run(n=0, per=7) == AADApiResult.OK  # launches nothing
        torch.cuda.synchronize()
        assert (out.bits() == CANARY).all()  # a refused call writes nothing
        for accepted in (dict(), dict(ga=None, gb=None, sp=None), dict(b=a, pb=T), dict(per=4), dict(per=1, sp=s + 8), dict(a=a + 2, b=b + 6)):
            assert run(**accepted) == AADApiResult.OK, accepted
        torch.cuda.synchronize()
        assert not out.bits().any()  # silence
    finally:
        lib.AADHip_SpectrogramDestroy(handle)


@pytest.mark.parametrize("name,channels", [("mixed", 1), ("mix", 1), ("mix", 2)], ids=["mono_corpus", "down_mix", "stereo"])
def test_mel_mix_windows(engine, corpora, name, channels):  # noqa: F811
    import torch
    from aad_amd.engine import mel_filters
    images, data, table, headers, rows = corpora[name]
    d_img = torch.from_numpy(data).cuda()
    sizes = [len(i) for i in images]
    s_windows = np.array([(1, 5), (2, 2500), (0, 0), (1, 1234), (2, 300)], dtype=np.int64)
    n_windows = np.array([(2, 100), (1, 0), (1, 2000), (0, 10), (2, 2950)], dtype=np.int64)
    frames, n_fft, W, H = 600, 256, 200, 80
    filters = mel_filters(16000, n_fft, 23)
    snr = torch.tensor([10.0, 0.0, -5.0, 20.0, 3.0], device="cuda")
    signal = (d_img, sizes, torch.from_numpy(s_windows).cuda())
    noise = (d_img, sizes, torch.from_numpy(n_windows).cuda())
    s_rows = _window_rows(rows[channels], s_windows, frames, channels)
    n_rows = _window_rows(rows[channels], n_windows, frames, channels)
    for spans in (None, [(300, 123), (frames, 0), (2 ** 63, 599), (77, 600), (1, 0)]):
        d_spans = _spans(torch, spans)
        got, gains = engine.mel_mix_windows(signal, noise, frames, snr, n_fft, H, filters, channels=channels, win_length=W, noise_spans=d_spans)
        assert got.shape == (5, channels, 1 + (frames - W) // H, 23) and got.is_contiguous()
        assert gains.shape == (5,) and gains.dtype == torch.float32 and bool((gains[:3] > 0).all())
        x = mo.mix_rows(s_rows.reshape(-1, frames), n_rows.reshape(-1, frames), channels, None, gains.cpu().numpy(), spans)
        want = so.spectrogram_rows(x.reshape(5, channels, frames), so.hann(W), n_fft, H, filters)
        _same(_bits(torch, got), want, ("mel_mix_windows", name, channels, spans is not None))
        floats, float_gains = engine.mix_windows(signal, noise, frames, snr, torch.float32, channels=channels, noise_spans=d_spans)
        assert torch.equal(float_gains, gains)
        if name == "mixed":  # no stereo to mono down-mix: the old path's float rows, quantised, hold the same samples
            quantised = torch.round(floats * 32768.0).clamp(-32768, 32767).to(torch.int16)
            assert np.array_equal(quantised.cpu().numpy().reshape(-1, frames), x)
            spec = engine.spectrogram(n_fft, H, W, filters=filters)
            try:
                assert np.array_equal(_bits(torch, spec.run(quantised)), _bits(torch, got))
            finally:
                spec.close()
