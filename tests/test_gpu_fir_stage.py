"""The seven calls of the FIR stages that launch (aad_amd/csrc/aad_fir_stage.hip: AADHip_ResamplerResolve, ...Run, ...RunGain,
...RunStats, AADHip_ConvolverResolve, ...Run, ...RunGain) through ctypes, each held to the one rule they share
(aad_fir_stage.h): a good call of 2 windows, 1 channel and 8 output frames - one ratio 1/1, one response {1.0} - and then the same
call spoiled one argument at a time.  Every spoiled call returns INVALID_ARGUMENT, leaves last_error beginning with the call's own
name and, after a synchronise, every output as the canaries it held: each refusal comes before the launch.  A Resolve has no
source rows, source_frames or channels: its source is the window table, its output the source windows and the lanes."""
import pytest

from aad_amd.capi import AADApiResult, SAMPLE_FLOAT32, WINDOW_GAIN_STORE
from test_gpu_resample_mix import CANARY, Bordered, _direct
from test_gpu_window_resample import engine  # noqa: F401

pytestmark = pytest.mark.gpu

N, CH, FRAMES = 2, 1, 8
ENTRIES = {  # entry point -> (its name in last_error, its arguments behind the handle, in order)
    "AADHip_ResamplerResolve": ("resampler resolve", ("n", "windows", "selector", "frames", "source_windows", "lanes_out")),
    "AADHip_ResamplerRun": ("resampler run", ("n", "channels", "source", "source_frames", "lanes", "frames", "type", "out")),
    "AADHip_ResamplerRunGain": ("resampler run with gain", ("n", "channels", "source", "source_frames", "lanes", "spans", "frames", "type",
                                                            "out", "gain", "mode")),
    "AADHip_ResamplerRunStats": ("resampler run with statistics", ("n", "channels", "source", "source_frames", "lanes", "source_stats",
                                                                   "spans", "frames", "type", "out", "stats")),
    "AADHip_ConvolverResolve": ("convolver resolve", ("n", "windows", "selector", "frames", "source_windows", "lanes_out")),
    "AADHip_ConvolverRun": ("convolver run", ("n", "channels", "source", "source_frames", "lanes", "frames", "type", "out")),
    "AADHip_ConvolverRunGain": ("convolver run with gain", ("n", "channels", "source", "source_frames", "lanes", "spans", "frames", "type",
                                                            "out", "gain", "mode")),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_spoiled_call_is_refused_by_name_and_writes_nothing(engine, entry):  # noqa: F811
    import torch
    what, names = ENTRIES[entry]
    resolve = entry.endswith("Resolve")
    stage = engine.resampler([(1, 1)], [[0]]) if "Resampler" in entry else engine.convolver([[1.0]])
    try:
        t_src = stage.source_frames(FRAMES)
        source = torch.full((N, CH, t_src), 7, dtype=torch.int16, device="cuda")
        outputs = {"out": Bordered(torch, (N, CH, FRAMES), "float32", CANARY["float32"]),
                   "source_windows": Bordered(torch, (N, 2), "int64", CANARY["int64"]),
                   "lanes_out": Bordered(torch, (N, 4), "int16", CANARY["int16"]),
                   "stats": Bordered(torch, (N, CH, 4), "int64", CANARY["int64"])}
        good_out = torch.zeros((N, CH, FRAMES), dtype=torch.float32, device="cuda")
        good_tables = torch.zeros((3, N, 4), dtype=torch.int64, device="cuda")  # source windows, lanes, statistics of the good call
        lanes = torch.zeros((N, 2), dtype=torch.int32, device="cuda")    # (bank or response 0, shift 0)
        windows = torch.zeros((N, 2), dtype=torch.int64, device="cuda")  # (stream 0, frame 0)
        source_stats = torch.zeros((N, CH, 4), dtype=torch.int64, device="cuda")
        values = {"n": N, "channels": CH, "frames": FRAMES, "source_frames": t_src, "type": SAMPLE_FLOAT32, "mode": WINDOW_GAIN_STORE,
                  "source": source.data_ptr(), "lanes": lanes.data_ptr(), "windows": windows.data_ptr(), "selector": None, "spans": None,
                  "gain": None, "source_stats": source_stats.data_ptr()}
        values.update({k: b.view.data_ptr() for k, b in outputs.items()})
        call = lambda v: _direct(engine, getattr(engine.lib, entry), stage.handle, *[v[k] for k in names])
        good = dict(values, out=good_out.data_ptr(), source_windows=good_tables[0].data_ptr(), lanes_out=good_tables[1].data_ptr(),
                    stats=good_tables[2].data_ptr())
        assert call(good) == AADApiResult.OK
        if not resolve:
            assert (good_out.cpu().numpy() != 0).all()  # rows of sevens through a filter with one dominant tap: the run wrote them
        spoiled = [("a null source", {"windows" if resolve else "source": None}),
                   ("out off by one byte", {"source_windows" if resolve else "out": values["source_windows" if resolve else "out"] + 1})]
        if not resolve:
            spoiled += [("source_frames one short", {"source_frames": t_src - 1}), ("0 channels", {"channels": 0})]
        if "mode" in names:
            spoiled.append(("mode 2", {"mode": 2}))
        for reason, change in spoiled:
            assert set(change) <= set(names), reason
            assert call(dict(values, **change)) == AADApiResult.INVALID_ARGUMENT, reason
            assert engine.last_error().startswith(what + ":"), (reason, engine.last_error())
            for name, buffer in outputs.items():
                assert (buffer.bits() == CANARY[buffer.name]).all(), (reason, name)
    finally:
        stage.close()
