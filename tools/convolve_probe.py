"""What reverberation costs (DESIGN.md "Reverberation"), in the style of tools/resample_probe.py.

Shape: --windows mono windows (default 1024) of --frames frames (default 64000) drawn from a 4-bit corpus on the device, convolved
with one response of --taps K (repeatable; default 512, 4096, 16384): an exponentially decaying noise tail behind a unit peak.
Per K, each step's time from HIP events recorded on the engine's stream around it, the median of --steps runs after --warmup with
min and max for the FIR:
  resolve   AADHip_ConvolverResolve
  decode    AADHip_WindowDecodePlanRun of the source windows, T_src frames, int16 - the source batch
  fir       AADHip_ConvolverRun into float32 rows, with the int8 multiply-accumulates per second it achieves: 4 N T K, the four
            byte products of every 16-bit product, the matrix's zero padding not counted
  fft       the composition the stage replaces: decode_windows into float32 rows of T + K - 1 frames' worth (here: the same source
            windows decoded as float32), torch.fft.rfft / irfft convolution with the float taps, crop and scale - timed by the
            host clock around the call and a synchronise, like the three steps together beside it
The first window's row is checked against tests/convolve_oracle.py.  Prints one line per K; --out appends them to a file.
--mix adds two lines per K, as resample_probe.py --mix does for the resample stage:
  fir variants   over one source batch decoded with statistics, timed in turn within each step (each behind an untimed plain run,
            so that all of them find the caches as the same kernel left them), median (min - max): the plain FIR into float32,
            AADHip_ConvolverRunStats without rows and with float32 rows, AADHip_ConvolverRunGain STORE and ADD
  mix       Engine.mix_windows_reverberated end to end (dry noise) against the composition it replaces - a float32
            decode_windows_reverberated batch, a float32 decode_windows batch, two vector_norm reductions and one addcmul -
            by the host clock, with the peak of torch's allocator above the result"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aad_amd.capi import SAMPLE_FLOAT32, make_parameter  # noqa: E402
from aad_amd.engine import Engine, _check  # noqa: E402
from aad_amd.synth import synth_pcm  # noqa: E402
from resample_probe import host_timed, pcm_decoded, timed, timed_all, timed_in_turn  # noqa: E402


def host_ms(steps, warmup, fn):
    ms = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def mix_rows(engine, args, conv, plan, data, size, windows, h, K, lines):
    """the two lines of --mix for one response"""
    lib = engine.lib
    n, frames, ch = args.windows, args.frames, 1
    source = conv.decode_source(plan, data, windows, frames, stats=True)
    out = torch.empty((n, ch, frames), dtype=torch.float32, device="cuda")
    stats = torch.empty((n, ch, 4), dtype=torch.int64, device="cuda")
    gain = torch.rand(n, device="cuda") + 0.5
    head = (conv.handle, n, ch, source.rows.data_ptr(), source.source_frames, source.lanes.data_ptr())
    run_stats = lambda rows: _check("AADHip_ConvolverRunStats", lib.AADHip_ConvolverRunStats(
        *head, source.stats.data_ptr(), None, frames, SAMPLE_FLOAT32, rows, stats.data_ptr()))
    run_gain = lambda mode: _check("AADHip_ConvolverRunGain", lib.AADHip_ConvolverRunGain(
        *head, None, frames, SAMPLE_FLOAT32, out.data_ptr(), gain.data_ptr(), mode))
    fns = (("plain", lambda: _check("AADHip_ConvolverRun", lib.AADHip_ConvolverRun(*head, frames, SAMPLE_FLOAT32, out.data_ptr()))),
           ("stats", lambda: run_stats(None)), ("stats + rows", lambda: run_stats(out.data_ptr())),
           ("gain", lambda: run_gain(0)), ("gain ADD", lambda: run_gain(1)))
    ms = timed_in_turn(engine.stream, args.steps, args.warmup, fns)
    lines.append("fir variants K=%d  N=%d C=%d T=%d  " % (K, n, ch, frames) + "  ".join(
        "%s %.3f ms (%.3f - %.3f)" % (name, statistics.median(v), min(v), max(v)) for name, v in ms.items()))
    print(lines[-1], flush=True)
    del source, out, stats
    noise_windows = windows.flip(0).contiguous()

    def mix():
        return engine.mix_windows_reverberated((data, size, windows), (data, size, noise_windows), frames, 6.0, [h])

    def composed():
        s = engine.decode_windows_reverberated(data, size, windows, frames, [h])
        z = engine.decode_windows(data, size, noise_windows, frames)
        p_s = torch.linalg.vector_norm(s, dim=(1, 2)).double().square()  # reductions without a temporary batch
        p_n = torch.linalg.vector_norm(z, dim=(1, 2)).double().square()
        g = torch.where(p_n > 0, (p_s / p_n.clamp(min=1e-300)).sqrt() * 10.0 ** (-6.0 / 20.0), torch.zeros_like(p_n)).float()
        return torch.addcmul(s, z, g[:, None, None]), g

    t_mix, peak_mix = host_timed(args.steps, args.warmup, mix)
    t_comp, peak_comp = host_timed(args.steps, args.warmup, composed)
    lines.append("mix K=%d  N=%d C=%d T=%d  mix_windows_reverberated %.3f ms, %.1f MB of temporaries  composed %.3f ms, %.1f MB of "
                 "temporaries" % (K, n, ch, frames, t_mix, peak_mix / 1e6, t_comp, peak_comp / 1e6))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=64000)
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--taps", type=int, action="append", help="a response length to time instead of 512, 4096 and 16384; repeatable")
    ap.add_argument("--out")
    ap.add_argument("--mix", action="store_true", help="add the lines of the FIR variants and of mix_windows_reverberated")
    args = ap.parse_args()
    import convolve_oracle as co
    engine = Engine(0, stream=None)
    lib = engine.lib
    n, frames, ch = args.windows, args.frames, 1
    samples = frames * 2 + 4096
    pcm = synth_pcm(args.streams, samples, ch, seed=5)
    lines = []
    with torch.cuda.stream(engine.stream):
        data, size = engine.encode_uniform(torch.from_numpy(pcm).cuda(), make_parameter(ch, 4, 1024, 16000, False, 0))
        plan = engine._corpus_window_plan(data, size, None)
        gen = torch.Generator(device="cuda").manual_seed(11)
        windows = torch.stack([torch.randint(0, args.streams, (n,), generator=gen, device="cuda"),
                               torch.randint(0, samples // 2, (n,), generator=gen, device="cuda")], dim=1).contiguous()
        for K in args.taps or [512, 4096, 16384]:
            rng = np.random.default_rng(K)
            h = (rng.uniform(-0.5, 0.5, size=K) * np.exp(-np.arange(K) * (6.9 / K))).astype(np.float32)  # -60 dB at the end
            h[0] = 1.0
            conv = engine.convolver([h])
            t_src = conv.source_frames(frames)
            src_windows = torch.empty((n, 2), dtype=torch.int64, device="cuda")
            lanes = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            rows = torch.empty((n, ch, t_src), dtype=torch.int16, device="cuda")
            out = torch.empty((n, ch, frames), dtype=torch.float32, device="cuda")
            resolve = lambda: _check("AADHip_ConvolverResolve", lib.AADHip_ConvolverResolve(
                conv.handle, n, windows.data_ptr(), None, frames, src_windows.data_ptr(), lanes.data_ptr()))
            decode = lambda: plan.run(data, src_windows, t_src, torch.int16, out=rows, ordered=False)
            fir = lambda: _check("AADHip_ConvolverRun", lib.AADHip_ConvolverRun(
                conv.handle, n, ch, rows.data_ptr(), t_src, lanes.data_ptr(), frames, SAMPLE_FLOAT32, out.data_ptr()))
            t = {name: timed(engine.stream, args.steps, args.warmup, fn) for name, fn in (("resolve", resolve), ("decode", decode))}
            fir_ms = timed_all(engine.stream, args.steps, args.warmup, fir)
            t["fir"] = statistics.median(fir_ms)

            def three_steps():
                resolve()
                decode()
                fir()

            d_taps = torch.from_numpy(h).cuda()
            size_fft = 1 << (t_src - 1).bit_length()

            def fft():
                # the same frames as the source batch, as float32; y[n] = sum_k h[k] x[K - 1 + n - k]
                x = plan.run(data, src_windows, t_src, torch.float32, ordered=False)
                y = torch.fft.irfft(torch.fft.rfft(x, size_fft) * torch.fft.rfft(d_taps, size_fft), size_fft)
                return y[..., K - 1:K - 1 + frames].contiguous()

            t["three"] = host_ms(args.steps, args.warmup, three_steps)
            t["fft"] = host_ms(args.steps, args.warmup, fft)
            q, d, taps = conv.response(0)
            s, f = (int(v) for v in windows[0].cpu())
            x = pcm_decoded(engine, data, size, s)[:, 0]
            want = co.element_bits(co.row(x, len(x), f, frames, (taps.astype(np.int64), q, d)), q, "float32")
            exact = bool((out[0, 0].cpu().numpy().view(np.uint32) == want).all())
            # how far the float32 FFT rows are from the exact ones (window 0 starts K - 1 frames into its source row, or at frame 0)
            shift = int(lanes[0, 1].cpu())
            err = float((fft()[0, 0, :frames].cpu() - torch.from_numpy(want.view(np.float32))).abs().max()) if shift == K - 1 else float("nan")
            macs = 4.0 * n * ch * frames * K
            lines.append("K=%d q=%d  N=%d C=%d T=%d T_src=%d  resolve %.4f ms  decode (int16 source batch) %.3f ms  fir %.3f ms (%.3f - %.3f) "
                         "%.1f T int8 MAC/s  three steps by the host clock %.3f ms  float32 decode + torch.fft %.3f ms (max |error| of its "
                         "rows %.2e)  exact=%s" % (K, q, n, ch, frames, t_src, t["resolve"], t["decode"], t["fir"], min(fir_ms), max(fir_ms),
                                                   macs / t["fir"] / 1e9, t["three"], t["fft"], err, exact))
            print(lines[-1], flush=True)
            del rows, out
            if args.mix:
                mix_rows(engine, args, conv, plan, data, size, windows, h, K, lines)
            conv.close()
        plan.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    engine.close()


if __name__ == "__main__":
    main()
