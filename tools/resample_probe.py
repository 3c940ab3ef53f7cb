"""What the resample stage costs next to the window decode it follows (DESIGN.md "Window decode at another rate").

Shape: --windows stereo windows (default 1024) of --frames output frames (default 48000) drawn from a 4-bit corpus on the device,
once at 147/160 (48 kHz to 44.1 kHz) and once at 160/147 - or at every --ratio UP/DOWN given, any ratio the constructor takes;
--wide builds the resamplers with AADHip_ResamplerCreateWide (DESIGN.md "Wide resampler"), which 1600/3969 needs.  Per ratio, each step's time from HIP events recorded on the engine's
stream around it, the median of --steps runs after --warmup:
  resolve   AADHip_ResamplerResolve
  decode    AADHip_WindowDecodePlanRun of the source windows, T_src frames, int16 - the source batch
  fir       AADHip_ResamplerRun into float32 rows, with the bytes it moves (the source batch read once, the rows written once)
  plain     AADHip_WindowDecodePlanRun of the same windows, T frames, float32: the path without resampling
The first window's row is checked against tests/resample_oracle.py.  Prints one line per ratio; --out appends them to a file.

--mix adds, at 147/160 (DESIGN.md "Resampled rows with gain, spans and statistics"):
  fir variants   AADHip_ResamplerRun, AADHip_ResamplerRunGain (float32, NULL spans: STORE with a gain table, STORE without one,
                 ADD) and a statistics-only AADHip_ResamplerRunStats over the same source batch, timed in turn within every step - median and min - max of each
                 (each behind an untimed plain run, so that all three find the caches as that run leaves them)
  mix            Engine.mix_windows_resampled end to end (host clock around the call and a synchronise) against the composition
                 without it: two Engine.decode_windows_resampled float32 batches, torch reductions for the levels and one
                 torch.addcmul - with the peak of torch's allocator above what was allocated before the call, less the result."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aad_amd.capi import SAMPLE_FLOAT32, make_parameter  # noqa: E402
from aad_amd.engine import Engine, _check  # noqa: E402
from aad_amd.synth import synth_pcm  # noqa: E402


def timed(stream, steps, warmup, fn):
    """median milliseconds of fn's work on `stream`, between two events recorded around it"""
    return statistics.median(timed_all(stream, steps, warmup, fn))


def timed_all(stream, steps, warmup, fn):
    """the milliseconds of each of `steps` runs of fn on `stream`"""
    ms = []
    for k in range(warmup + steps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        fn()
        stop.record(stream)
        stop.synchronize()
        if k >= warmup:
            ms.append(start.elapsed_time(stop))
    return ms


def timed_in_turn(stream, steps, warmup, fns):
    """{name: [ms per step]}: every step times each fn once, so that drift falls on all of them alike, and each behind an
    untimed run of the first fn: what the kernel before left in the caches counts (a run that stores nothing leaves the source
    batch there), so all of them follow the same one"""
    ms = {name: [] for name, _ in fns}
    for k in range(warmup + steps):
        for name, fn in fns:
            fns[0][1]()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            fn()
            stop.record(stream)
            stop.synchronize()
            if k >= warmup:
                ms[name].append(start.elapsed_time(stop))
    return ms


def host_timed(steps, warmup, fn):
    """-> (median ms of fn() + synchronise by the host clock, peak bytes of torch's allocator above the start less the result's)"""
    import time
    ms, peak = [], 0
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
        kept = sum(t.numel() * t.element_size() for t in (result if isinstance(result, tuple) else (result,)))
        peak = max(peak, torch.cuda.max_memory_allocated() - before - kept)
        del result
    return statistics.median(ms), peak


def mix_rows(engine, args, plan, data, size, windows, lines):
    """the three rows of --mix, at 147/160"""
    lib = engine.lib
    n, frames, ch = args.windows, args.frames, 2
    res = make_resampler(engine, args, (147, 160))
    source = res.decode_source(plan, data, windows, frames, stats=True)
    t_src = source.source_frames
    out = torch.empty((n, ch, frames), dtype=torch.float32, device="cuda")
    stats = torch.empty((n, ch, 4), dtype=torch.int64, device="cuda")
    gain = torch.rand(n, device="cuda") + 0.5
    head = (res.handle, n, ch, source.rows.data_ptr(), t_src, source.lanes.data_ptr())
    fns = (("plain", lambda: _check("AADHip_ResamplerRun", lib.AADHip_ResamplerRun(*head, frames, SAMPLE_FLOAT32, out.data_ptr()))),
           ("gain", lambda: _check("AADHip_ResamplerRunGain", lib.AADHip_ResamplerRunGain(
               *head, None, frames, SAMPLE_FLOAT32, out.data_ptr(), gain.data_ptr(), 0))),
           ("gain no table", lambda: _check("AADHip_ResamplerRunGain", lib.AADHip_ResamplerRunGain(
               *head, None, frames, SAMPLE_FLOAT32, out.data_ptr(), None, 0))),
           ("gain ADD", lambda: _check("AADHip_ResamplerRunGain", lib.AADHip_ResamplerRunGain(
               *head, None, frames, SAMPLE_FLOAT32, out.data_ptr(), gain.data_ptr(), 1))),
           ("stats", lambda: _check("AADHip_ResamplerRunStats", lib.AADHip_ResamplerRunStats(
               *head, source.stats.data_ptr(), None, frames, SAMPLE_FLOAT32, None, stats.data_ptr()))))
    ms = timed_in_turn(engine.stream, args.steps, args.warmup, fns)
    lines.append("fir variants 147/160%s  N=%d C=%d T=%d  " % (" wide" if args.wide else "", n, ch, frames) + "  ".join(
        "%s %.3f ms (%.3f - %.3f)" % (name, statistics.median(v), min(v), max(v)) for name, v in ms.items()))
    print(lines[-1], flush=True)
    res.close()
    del source, out, stats
    noise_windows = windows.flip(0).contiguous()
    sizes = size

    def mix():
        return engine.mix_windows_resampled((data, sizes, windows), (data, sizes, noise_windows), frames, 6.0, 44100)

    def composed():
        s = engine.decode_windows_resampled(data, sizes, windows, frames, 44100)
        z = engine.decode_windows_resampled(data, sizes, noise_windows, frames, 44100)
        p_s = torch.linalg.vector_norm(s, dim=(1, 2)).double().square()  # reductions without a temporary batch
        p_n = torch.linalg.vector_norm(z, dim=(1, 2)).double().square()
        g = torch.where(p_n > 0, (p_s / p_n.clamp(min=1e-300)).sqrt() * 10.0 ** (-6.0 / 20.0), torch.zeros_like(p_n)).float()
        return torch.addcmul(s, z, g[:, None, None]), g

    t_mix, peak_mix = host_timed(args.steps, args.warmup, mix)
    t_comp, peak_comp = host_timed(args.steps, args.warmup, composed)
    lines.append("mix 147/160  N=%d C=%d T=%d  mix_windows_resampled %.3f ms, %.1f MB of temporaries  composed %.3f ms, %.1f MB of "
                 "temporaries" % (n, ch, frames, t_mix, peak_mix / 1e6, t_comp, peak_comp / 1e6))
    print(lines[-1], flush=True)


def make_resampler(engine, args, ratio):
    """one bank for every stream; the plain call is made as it always was"""
    select = [[0]] * args.streams
    return engine.resampler([ratio], select, wide=True) if args.wide else engine.resampler([ratio], select)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--mix", action="store_true", help="add the rows of the FIR variants and of mix_windows_resampled")
    ap.add_argument("--wide", action="store_true", help="build the resamplers with AADHip_ResamplerCreateWide")
    ap.add_argument("--ratio", action="append", metavar="UP/DOWN", help="a ratio to time instead of 147/160 and 160/147; repeatable")
    args = ap.parse_args()
    ratios = [tuple(int(v) for v in r.split("/")) for r in args.ratio] if args.ratio else [(147, 160), (160, 147)]
    engine = Engine(0, stream=None)
    lib = engine.lib
    n, frames, ch = args.windows, args.frames, 2
    steepest = max([160 / 147] + [down / up for up, down in ratios])
    samples = int(frames * steepest) * 2 + 4096  # every window lies inside its stream at every ratio
    pcm = synth_pcm(args.streams, samples, ch, seed=5)
    lines = []
    with torch.cuda.stream(engine.stream):
        data, size = engine.encode_uniform(torch.from_numpy(pcm).cuda(), make_parameter(ch, 4, 1024, 48000, False, 0))
        plan = engine._corpus_window_plan(data, size, None)
        gen = torch.Generator(device="cuda").manual_seed(11)
        windows = torch.stack([torch.randint(0, args.streams, (n,), generator=gen, device="cuda"),
                               torch.randint(0, samples // 2 - 4096, (n,), generator=gen, device="cuda")], dim=1).contiguous()
        for ratio in ratios:
            res = make_resampler(engine, args, ratio)
            t_src = res.source_frames(frames)
            src_windows = torch.empty((n, 2), dtype=torch.int64, device="cuda")
            lanes = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            rows = torch.empty((n, ch, t_src), dtype=torch.int16, device="cuda")
            out = torch.empty((n, ch, frames), dtype=torch.float32, device="cuda")
            plain = torch.empty((n, ch, frames), dtype=torch.float32, device="cuda")
            resolve = lambda: _check("AADHip_ResamplerResolve", lib.AADHip_ResamplerResolve(
                res.handle, n, windows.data_ptr(), None, frames, src_windows.data_ptr(), lanes.data_ptr()))
            decode = lambda: plan.run(data, src_windows, t_src, torch.int16, out=rows, ordered=False)
            fir = lambda: _check("AADHip_ResamplerRun", lib.AADHip_ResamplerRun(
                res.handle, n, ch, rows.data_ptr(), t_src, lanes.data_ptr(), frames, SAMPLE_FLOAT32, out.data_ptr()))
            decode_plain = lambda: plan.run(data, windows, frames, torch.float32, out=plain, ordered=False)
            t = {name: timed(engine.stream, args.steps, args.warmup, fn) for name, fn in (("resolve", resolve), ("decode", decode))}
            fir_ms = timed_all(engine.stream, args.steps, args.warmup, fir)
            t["fir"] = statistics.median(fir_ms)
            t["plain"] = timed(engine.stream, args.steps, args.warmup, decode_plain)
            t["plain again"] = timed(engine.stream, args.steps, args.warmup, decode_plain)  # drift between the first and the last
            moved = n * ch * (t_src * 2 + frames * 4)
            import resample_oracle as ro
            L, M, h = res.bank(0)
            s, f = (int(v) for v in windows[0].cpu())
            want = ro.convert(ro.fir(pcm_decoded(engine, data, size, s)[:, 0], f, frames, L, M, h), "float32")
            exact = bool((out[0, 0].cpu().numpy().view(np.uint32) == want).all())
            lines.append("ratio %d/%d%s K=%d  N=%d C=%d T=%d T_src=%d  resolve %.4f ms  decode (int16 source batch) %.3f ms  fir %.3f ms (%.3f - %.3f) "
                         "(%.1f MB moved, %.0f GB/s)  three steps %.3f ms  plain float32 decode %.3f ms (again %.3f)  fir / decode %.2f  "
                         "exact=%s" % (ratio[0], ratio[1], " wide" if args.wide else "", h.shape[1], n, ch, frames, t_src, t["resolve"], t["decode"], t["fir"], min(fir_ms), max(fir_ms), moved / 1e6,
                                       moved / t["fir"] / 1e6, t["resolve"] + t["decode"] + t["fir"], t["plain"], t["plain again"],
                                       t["fir"] / t["decode"], exact))
            print(lines[-1], flush=True)
            res.close()
        if args.mix:
            mix_rows(engine, args, plan, data, size, windows, lines)
        plan.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    engine.close()


def pcm_decoded(engine, data, size, stream):
    """one stream's whole decode, int16 [samples, channels], from the device decoder"""
    dec, _ = engine.decode_uniform(data[stream:stream + 1], size)
    return dec[0].cpu().numpy()


if __name__ == "__main__":
    main()
