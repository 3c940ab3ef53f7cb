"""The Python level of the spectrogram stage's mix (Spectrogram.run_mix, Engine.mel_mix_windows; aad_amd/engine.py) over the
library that records its calls (tests/test_spectrogram_engine_host.py, tests/test_engine_tensor_contract.py): what reaches
AADHip_SpectrogramRunMix for contiguous, pitched and sliced operands, one refusal per rule raised before any library call, and
mel_mix_windows' five runs - statistics, statistics, decode, decode, mix - in their order with their arguments.  No GPU."""
import numpy as np
import pytest
import torch

from test_engine_tensor_contract import CH, header_bytes
from test_spectrogram_engine_host import BINS, F, HOP, MELS, N, N_FFT, T, WIN, _filters, engine  # noqa: F401

MIX = "AADHip_SpectrogramRunMix"


def _i16(*shape):
    return torch.zeros(shape, dtype=torch.int16)


def test_run_mix_hands_over_both_batches_gains_and_spans(engine):  # noqa: F811
    spec = engine.spectrogram(N_FFT, HOP, WIN, filters=_filters())
    rows, other = _i16(N, CH, T), _i16(N, CH, T)
    gain, other_gain, spans = torch.ones(N), torch.ones(N), torch.zeros((N, 2), dtype=torch.int64)
    out = spec.run_mix(rows, other, gain, other_gain, spans)
    assert tuple(out.shape) == (N, CH, F, MELS) and out.dtype == torch.float32 and out.is_contiguous()
    assert engine.lib.last(MIX) == (spec.handle, N * CH, rows.data_ptr(), T, other.data_ptr(), T, CH, gain.data_ptr(), other_gain.data_ptr(),
                                    spans.data_ptr(), T, out.data_ptr())
    # no tables: NULL pointers; an `out` of the caller's
    given = torch.zeros((N, CH, F, MELS))
    assert spec.run_mix(rows, other, out=given) is given
    assert engine.lib.last(MIX) == (spec.handle, N * CH, rows.data_ptr(), T, other.data_ptr(), T, CH, None, None, None, T, given.data_ptr())
    # [R, T]: a gain pair per row; each operand a slice of longer rows read where it lies, each with a pitch of its own
    wide_a, wide_b = _i16(N, T + 9), _i16(N, T + 40)
    spec.run_mix(wide_a[:, 2:2 + T], wide_b[:, 33:33 + T], other_gain=other_gain)
    assert engine.lib.last(MIX)[1:11] == (N, wide_a.data_ptr() + 4, T + 9, wide_b.data_ptr() + 66, T + 40, 1, None, other_gain.data_ptr(), None, T)
    # [N, C, T] with every row further apart; [N, 1, T] takes its pitch from the windows; the same memory twice
    big = _i16(N, CH, T + 5)
    spec.run_mix(big[..., :T], other)
    assert engine.lib.last(MIX)[1:7] == (N * CH, big.data_ptr(), T + 5, other.data_ptr(), T, CH)
    spec.run_mix(rows[:, :1], big[:, :1, 3:3 + T], gain)
    assert engine.lib.last(MIX)[1:8] == (N, rows.data_ptr(), CH * T, big.data_ptr() + 6, CH * (T + 5), 1, gain.data_ptr())
    spec.run_mix(rows, rows)
    assert engine.lib.last(MIX)[2:6] == (rows.data_ptr(), T, rows.data_ptr(), T)
    # no rows: no call
    before = len(engine.lib.calls)
    assert tuple(spec.run_mix(_i16(0, T), _i16(0, T)).shape) == (0, F, MELS)
    assert engine.lib.calls[before:] == []


GOOD = dict(rows=lambda: _i16(N, CH, T), other=lambda: _i16(N, CH, T), gain=lambda: None, other_gain=lambda: None, spans=lambda: None,
            out=lambda: None)
REFUSALS = [
    (dict(other=lambda: _i16(N, CH, T + 1)), "other: shape"),
    (dict(other=lambda: _i16(N * CH, T)), "other: shape"),
    (dict(other=lambda: torch.zeros((N, CH, T), dtype=torch.float32)), "other: dtype"),
    (dict(rows=lambda: torch.zeros((N, CH, T), dtype=torch.int32)), "rows: dtype"),
    (dict(other=lambda: np.zeros((N, CH, T), dtype=np.int16)), "other: a torch tensor"),
    (dict(other=lambda: torch.zeros((N, CH, T), dtype=torch.int16, device="meta")), "other: a tensor on the engine's device"),
    (dict(rows=lambda: _i16(N, CH, WIN - 1), other=lambda: _i16(N, CH, WIN - 1)), "rows: .* below the window"),
    (dict(other=lambda: _i16(N, CH, 2 * T)[..., ::2]), r"other: stride\(-1\) == 1"),
    (dict(other=lambda: _i16(N, CH + 1, T)[:, :CH]), "other: one pitch"),
    (dict(other=lambda: _i16(CH, T)[None].expand(N, CH, T)), "other: one pitch"),
    (dict(gain=lambda: torch.ones(N * CH)), "gain: shape"),
    (dict(other_gain=lambda: torch.ones((N, 1))), "other_gain: shape"),
    (dict(gain=lambda: torch.ones(N, dtype=torch.float64)), "gain: dtype"),
    (dict(other_gain=lambda: torch.ones(N, device="meta")), "other_gain: a tensor on the engine's device"),
    (dict(other_gain=lambda: torch.ones(2 * N)[::2]), "other_gain: a contiguous"),
    (dict(spans=lambda: torch.zeros((N, 3), dtype=torch.int64)), "spans: shape"),
    (dict(spans=lambda: torch.zeros((N * CH, 2), dtype=torch.int64)), "spans: shape"),
    (dict(spans=lambda: torch.zeros((N, 2), dtype=torch.int32)), "spans: dtype"),
    (dict(spans=lambda: torch.zeros((N, 2), dtype=torch.int64, device="meta")), "spans: a tensor on the engine's device"),
    (dict(spans=lambda: torch.zeros((N, 4), dtype=torch.int64)[:, ::2]), "spans: a contiguous"),
    (dict(out=lambda: torch.zeros((N, CH, F + 1, MELS))), "out: shape"),
    (dict(out=lambda: torch.zeros((N, CH, F, MELS), dtype=torch.float64)), "out: dtype"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=["%d-%s" % (i, r[1][:14].replace(": ", "-").replace(" ", "_")) for i, r in enumerate(REFUSALS)])
def test_run_mix_refuses_a_tensor_off_its_contract(engine, change, message):  # noqa: F811
    spec = engine.spectrogram(N_FFT, HOP, WIN, filters=_filters())
    args = {k: v() for k, v in dict(GOOD, **change).items()}
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match=message):
        spec.run_mix(**args)
    assert engine.lib.calls[before:] == []


def test_mel_mix_windows_runs_statistics_gains_decodes_and_one_mix(engine):  # noqa: F811
    from aad_amd import capi
    data = torch.zeros((3, 64), dtype=torch.uint8)
    data[:, :31] = torch.frombuffer(bytearray(header_bytes(CH, 100)), dtype=torch.uint8)
    noise_data = data.clone()
    s_windows, n_windows = torch.zeros((N, 2), dtype=torch.int64), torch.ones((N, 2), dtype=torch.int64)
    spans = torch.zeros((N, 2), dtype=torch.int64)
    f = _filters()
    out, gains = engine.mel_mix_windows((data, 64, s_windows), (noise_data, 64, n_windows), T, 10.0, N_FFT, HOP, f, win_length=WIN, noise_spans=spans)
    assert tuple(out.shape) == (N, CH, F, MELS) and out.dtype == torch.float32
    assert tuple(gains.shape) == (N,) and gains.dtype == torch.float32
    runs = [c for c in engine.lib.calls if "Run" in c[0]]
    assert [c[0] for c in runs] == ["AADHip_WindowDecodePlanRunStats", "AADHip_WindowDecodePlanRunPlacedStats",
                                    "AADHip_WindowDecodePlanRun", "AADHip_WindowDecodePlanRun", MIX]
    names = [c[0] for c in engine.lib.calls]
    assert names.index("AADHip_SpectrogramCreate") < names.index(runs[0][0])  # everything is built before anything runs
    assert names[-3:] == ["AADHip_SpectrogramDestroy", "AADHip_WindowDecodePlanDestroy", "AADHip_WindowDecodePlanDestroy"]
    s_stats, n_stats, s_decode, n_decode, mix = (c[1] for c in runs)
    s_plan, n_plan = s_stats[0], n_stats[0]
    assert s_plan != n_plan and (s_decode[0], n_decode[0]) == (s_plan, n_plan)
    # the signal's levels over its whole rows and no rows: (plan, data, N, windows, T, sample type, out, stats); the noise's over
    # its spans: (plan, data, N, windows, spans, T, stats)
    assert s_stats[1:5] == (data.data_ptr(), N, s_windows.data_ptr(), T) and s_stats[6] is None
    assert n_stats[1:6] == (noise_data.data_ptr(), N, n_windows.data_ptr(), spans.data_ptr(), T)
    # (plan, data, N, windows, T, sample type, out): two int16 batches
    assert s_decode[1:6] == (data.data_ptr(), N, s_windows.data_ptr(), T, capi.SAMPLE_INT16)
    assert n_decode[1:6] == (noise_data.data_ptr(), N, n_windows.data_ptr(), T, capi.SAMPLE_INT16)
    assert s_decode[6] != n_decode[6]
    # the signal at gain 1 (NULL), the noise at snr_gains' gains over its spans, a gain pair per window of C rows
    assert mix[1:] == (N * CH, s_decode[6], T, n_decode[6], T, CH, None, gains.data_ptr(), spans.data_ptr(), T, out.data_ptr())
    # without spans: NULL in the statistics run and in the mix; channels=1: one row per window
    out, gains = engine.mel_mix_windows((data, 64, s_windows), (noise_data, 64, n_windows), T, 10.0, N_FFT, HOP, None, channels=1)
    assert tuple(out.shape) == (N, 1, 1 + (T - N_FFT) // HOP, BINS)
    runs = [c for c in engine.lib.calls if "Run" in c[0]][-5:]
    assert [c[0] for c in runs][:2] == ["AADHip_WindowDecodePlanRunStats"] * 2 and runs[4][1][6:10] == (1, None, gains.data_ptr(), None)
    # a refused argument is found before anything is built
    before = len(engine.lib.calls)
    good = dict(signal=(data, 64, s_windows), noise=(noise_data, 64, n_windows), frames=T, snr_db=10.0, n_fft=N_FFT, hop=HOP, filters=f, win_length=WIN)
    for bad, message in ((dict(signal=(data, 64, s_windows.to(torch.int32))), "windows: dtype"),
                         (dict(noise=(noise_data, 64, torch.zeros((N + 1, 2), dtype=torch.int64))), "windows: shape"),
                         (dict(noise_spans=torch.zeros((N, 3), dtype=torch.int64)), "spans: shape"),
                         (dict(frames=WIN - 1), "frames"), (dict(n_fft=8192), "n_fft"), (dict(hop=0), "n_fft"),
                         (dict(filters=np.ones((MELS, BINS + 1))), "filters"), (dict(window=np.ones(WIN + 1)), "window")):
        with pytest.raises(ValueError, match=message):
            engine.mel_mix_windows(**dict(good, **bad))
    assert engine.lib.calls[before:] == []
