"""The Python level of the spectrogram stage (Engine.spectrogram, Spectrogram.run, Engine.mel_windows, mel_filters, frame_counts;
aad_amd/engine.py) over the library that records its calls (tests/test_engine_tensor_contract.py): what reaches the C calls and
in which order, one refusal per rule raised before any library call, frame_counts against a brute force and mel_filters against
its formula restated in tests/spectrogram_oracle.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrogram_oracle as so
from aad_amd.engine import frame_counts, mel_filters
from test_engine_tensor_contract import CH, CpuEngine, FakeLib, header_bytes

N_FFT, WIN, HOP, MELS = 64, 48, 16, 6
BINS = N_FFT // 2 + 1
N, T = 5, 48 + 16 * 9 + 7  # F = 10
F = 10


class SpectrogramFakeLib(FakeLib):
    """FakeLib whose spectrogram hands out a handle"""

    def __getattr__(self, name):
        call = FakeLib.__getattr__(self, name)

        def wrapped(*args):
            rc = call(*args)
            if name == "AADHip_SpectrogramCreate":
                args[-1]._obj.value = 0x7200
            return rc
        return wrapped


@pytest.fixture
def engine():
    e = CpuEngine.__new__(CpuEngine)
    e.torch, e.lib, e.device, e._ctx = torch, SpectrogramFakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def _filters():
    return mel_filters(16000, N_FFT, MELS)


def test_create_hands_over_shape_window_and_filters(engine):
    f = _filters()
    spec = engine.spectrogram(N_FFT, HOP, WIN, filters=f)
    args = engine.lib.last("AADHip_SpectrogramCreate")
    assert list(args[1:4]) == [N_FFT, WIN, HOP] and args[5] == MELS
    assert np.array_equal(np.frombuffer(C.string_at(args[4], 4 * WIN), dtype=np.float32), so.hann(WIN))  # the periodic Hann window
    assert np.array_equal(np.frombuffer(C.string_at(args[6], 4 * MELS * BINS), dtype=np.float32).reshape(MELS, BINS), f)
    assert (spec.columns, spec.bins, spec.win_length) == (MELS, BINS, WIN)
    plain = engine.spectrogram(N_FFT, HOP, window=np.ones(N_FFT))
    args = engine.lib.last("AADHip_SpectrogramCreate")
    assert list(args[1:4]) == [N_FFT, N_FFT, HOP] and args[5] == 0 and args[6] is None and plain.columns == BINS
    before = len(engine.lib.calls)
    for bad, message in ((dict(n_fft=8192), "n_fft"), (dict(win_length=N_FFT + 1), "n_fft"), (dict(win_length=0), "n_fft"), (dict(hop=0), "n_fft"),
                         (dict(window=np.ones(WIN + 1)), "window"), (dict(window=np.full(WIN, np.nan)), "window"),
                         (dict(filters=np.ones((MELS, BINS + 1))), "filters"), (dict(filters=np.ones(BINS)), "filters"),
                         (dict(filters=np.zeros((0, BINS))), "filters"), (dict(filters=np.full((1, BINS), np.inf)), "filters"),
                         (dict(filters=np.full((1, BINS), 2.0 ** -61)), "filters")):
        args = dict(dict(n_fft=N_FFT, hop=HOP, win_length=WIN), **bad)
        with pytest.raises(ValueError, match=message):
            engine.spectrogram(**args)
    assert engine.lib.calls[before:] == []
    spec.close()
    assert engine.lib.calls[-1][0] == "AADHip_SpectrogramDestroy" and spec.handle is None


def test_run_hands_over_rows_pitch_and_out(engine):
    spec = engine.spectrogram(N_FFT, HOP, WIN, filters=_filters())
    rows = torch.zeros((N, CH, T), dtype=torch.int16)
    out = spec.run(rows)
    assert tuple(out.shape) == (N, CH, F, MELS) and out.dtype == torch.float32 and out.is_contiguous()
    assert engine.lib.last("AADHip_SpectrogramRun") == (spec.handle, N * CH, rows.data_ptr(), T, T, out.data_ptr())
    # [R, T]; a slice of longer rows is read where it lies: pitch T + 9, and an `out` of the caller's
    wide = torch.zeros((N, T + 9), dtype=torch.int16)
    given = torch.zeros((N, F, MELS))
    assert spec.run(wide[:, 2:2 + T], out=given) is given
    assert engine.lib.last("AADHip_SpectrogramRun") == (spec.handle, N, wide.data_ptr() + 4, T + 9, T, given.data_ptr())
    # [N, C, T] with every row further apart; [N, 1, T] takes its pitch from the windows; one row has no pitch to speak of
    big = torch.zeros((N, CH, T + 5), dtype=torch.int16)
    spec.run(big[..., :T])
    assert engine.lib.last("AADHip_SpectrogramRun")[1:5] == (N * CH, big.data_ptr(), T + 5, T)
    spec.run(big[:, :1, 3:3 + T])
    assert engine.lib.last("AADHip_SpectrogramRun")[1:5] == (N, big.data_ptr() + 6, CH * (T + 5), T)
    spec.run(big[:1, :1, :T])
    assert engine.lib.last("AADHip_SpectrogramRun")[1:5] == (1, big.data_ptr(), T, T)
    # no rows: no call
    before = len(engine.lib.calls)
    assert tuple(spec.run(torch.zeros((0, T), dtype=torch.int16)).shape) == (0, F, MELS)
    assert engine.lib.calls[before:] == []
    assert spec.frames(T) is not None and engine.lib.calls[-1][0] == "AADHip_SpectrogramFrames"


REFUSALS = [
    (lambda: torch.zeros((N, CH, T), dtype=torch.float32), None, "rows: dtype"),
    (lambda: torch.zeros((N, CH, T), dtype=torch.int16, device="meta"), None, "rows: a tensor on the engine's device"),
    (lambda: torch.zeros(T, dtype=torch.int16), None, r"rows: \[N, C, T\] or \[R, T\]"),
    (lambda: torch.zeros((2, N, CH, T), dtype=torch.int16), None, r"rows: \[N, C, T\] or \[R, T\]"),
    (lambda: torch.zeros((N, CH, WIN - 1), dtype=torch.int16), None, "rows: .* below the window"),
    (lambda: torch.zeros((N, CH, 2 * T), dtype=torch.int16)[..., ::2], None, r"rows: stride\(-1\) == 1"),
    (lambda: torch.zeros((N, CH + 1, T), dtype=torch.int16)[:, :CH], None, "rows: one pitch"),
    (lambda: torch.zeros((CH, T), dtype=torch.int16)[None].expand(N, CH, T), None, "rows: one pitch"),
    (lambda: torch.zeros(T, dtype=torch.int16)[None].expand(N, T), None, "rows: a row pitch of at least"),
    (lambda: torch.zeros((N, CH, T), dtype=torch.int16), lambda: torch.zeros((N, CH, F, MELS), dtype=torch.float64), "out: dtype"),
    (lambda: torch.zeros((N, CH, T), dtype=torch.int16), lambda: torch.zeros((N, CH, F + 1, MELS)), "out: shape"),
    (lambda: torch.zeros((N, CH, T), dtype=torch.int16), lambda: torch.zeros((N * CH, F, MELS)), "out: shape"),
    (lambda: torch.zeros((N, CH, T), dtype=torch.int16), lambda: torch.zeros((N, CH, F, MELS + 2))[..., :MELS], "out: shape|out: a contiguous"),
    (lambda: torch.zeros((N, CH, T), dtype=torch.int16), lambda: torch.zeros((N, CH, F, MELS), device="meta"), "out: a tensor on the engine's device"),
]


@pytest.mark.parametrize("rows,out,message", REFUSALS, ids=["%d-%s" % (i, r[2][:12].replace(": ", "-").replace(" ", "_")) for i, r in enumerate(REFUSALS)])
def test_run_refuses_a_tensor_off_its_contract(engine, rows, out, message):
    spec = engine.spectrogram(N_FFT, HOP, WIN, filters=_filters())
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match=message):
        spec.run(rows(), out=None if out is None else out())
    assert engine.lib.calls[before:] == []


def test_mel_windows_decodes_int16_rows_then_runs_the_stage(engine):
    from aad_amd import capi
    data = torch.zeros((3, 64), dtype=torch.uint8)
    data[:, :31] = torch.frombuffer(bytearray(header_bytes(CH, 100)), dtype=torch.uint8)
    windows = torch.zeros((N, 2), dtype=torch.int64)
    f = _filters()
    out = engine.mel_windows(data, 64, windows, T, N_FFT, HOP, f, win_length=WIN)
    assert tuple(out.shape) == (N, CH, F, MELS) and out.dtype == torch.float32
    names = [c[0] for c in engine.lib.calls]
    assert names.index("AADHip_MixedWindowDecodePlanCreate") < names.index("AADHip_SpectrogramCreate") \
        < names.index("AADHip_WindowDecodePlanRun") < names.index("AADHip_SpectrogramRun")
    assert names[-2:] == ["AADHip_SpectrogramDestroy", "AADHip_WindowDecodePlanDestroy"]
    decode, run = engine.lib.last("AADHip_WindowDecodePlanRun"), engine.lib.last("AADHip_SpectrogramRun")
    assert decode[2:6] == (N, windows.data_ptr(), T, capi.SAMPLE_INT16)
    assert run[1:5] == (N * CH, decode[6], T, T) and run[5] == out.data_ptr()
    # channels=1: the channel-mix plan, one row per window; no filters: the power spectrum
    out = engine.mel_windows(data, 64, windows, T, N_FFT, HOP, None, channels=1)
    assert tuple(out.shape) == (N, 1, 1 + (T - N_FFT) // HOP, BINS)
    assert "AADHip_ChannelMixWindowDecodePlanCreate" in [c[0] for c in engine.lib.calls]
    # a refused argument is found before anything is built
    before = len(engine.lib.calls)
    for bad, message in ((dict(windows=windows.to(torch.int32)), "windows: dtype"), (dict(windows=torch.zeros((N, 3), dtype=torch.int64)), "windows: shape"),
                         (dict(frames=WIN - 1), "frames"), (dict(n_fft=8192), "n_fft"), (dict(hop=0), "n_fft"),
                         (dict(filters=np.ones((MELS, BINS + 1))), "filters"), (dict(window=np.ones(WIN + 1)), "window"),
                         (dict(data=torch.zeros((3, 64), dtype=torch.int8)), "data")):
        args = dict(dict(data=data, image_sizes=64, windows=windows, frames=T, n_fft=N_FFT, hop=HOP, filters=f, win_length=WIN), **bad)
        with pytest.raises(ValueError, match=message):
            engine.mel_windows(**args)
    assert engine.lib.calls[before:] == []


def test_frame_counts_against_a_brute_force():
    for W, H in ((400, 160), (80, 37), (16, 1), (5, 9)):
        counts = np.arange(0, W + 4 * H + 3)
        want = [so.frame_counts(int(c), W, H) for c in counts]
        assert frame_counts(counts, W, H).tolist() == want
        got = frame_counts(torch.from_numpy(counts), W, H)
        assert got.dtype == torch.int64 and got.tolist() == want
        # the count column of a statistics table, [N, C, 4]
        stats = torch.zeros((len(counts), 2, 4), dtype=torch.int64)
        stats[:, :, 3] = torch.from_numpy(counts)[:, None]
        assert frame_counts(stats[..., 3], W, H)[:, 1].tolist() == want
    assert int(frame_counts(4000, 400, 160)) == 23
    with pytest.raises(ValueError):
        frame_counts(10, 0, 1)


def test_mel_filters_against_the_formula_restated():
    for rate, n_fft, n_mels, f_min, f_max in ((16000, 512, 80, 0.0, None), (16000, 400, 40, 20.0, 7600.0), (44100, 2048, 128, 0.0, None),
                                              (8000, 96, 5, 100.0, 3000.0)):
        got, want = mel_filters(rate, n_fft, n_mels, f_min, f_max), so.mel_filters(rate, n_fft, n_mels, f_min, f_max)
        assert got.dtype == np.float32 and got.shape == want.shape == (n_mels, n_fft // 2 + 1)
        # both in float64 from the same formula; numpy's vector pow and Python's may differ in the last bit of a point
        assert np.allclose(got, want, rtol=2.0 ** -22, atol=2.0 ** -40)
        assert ((got > 2.0 ** -30) == (want > 2.0 ** -30)).all()
        nz = np.abs(got[got != 0])
        assert nz.min() >= 2.0 ** -60 and got.min() >= 0 and got.max() <= 1
    with pytest.raises(ValueError):
        mel_filters(16000, 512, 0)
    with pytest.raises(ValueError):
        mel_filters(16000, 512, 80, 9000.0)
