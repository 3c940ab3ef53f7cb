"""Planar encode against the interleaved path (profiles/r05_planar_encode.txt, DESIGN.md "Planar encode").

Kernel rows: the kernel's own time from the events AADHip_ContextSignalNextRun attaches to its dispatch, median of --reps runs,
for the interleaved plan (AADHip_EncodePlanRun on [N, T, C] int16) and planar plans over the same samples as [N, C, T] int16
and float32 (sample / 32768, which q maps back exactly).  Every planar image is compared with the interleaved one on the device.
  headline   1000 stereo 4-bit one-block streams, trials 0 and 2 (bench.py's shape)
  saturated  262 144 stereo 4-bit one-block streams (524 288 recurrences)
Corpus row (--corpus): 1000 stereo 60 s streams at 48 kHz as float32 [N, C, T], segmented L = 64, W = 8 -
Engine.encode_planar against the torch composite (convert, interleave, Engine.encode_uniform): wall time of the call (median of
three, synchronised) and the peak of torch.cuda.max_memory_allocated above input + images.
Prints one line per row; --out appends them to a file."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aad_amd.capi import LegacyCodec, make_parameter  # noqa: E402
from aad_amd.engine import Engine, HipEvent  # noqa: E402


def kernel_ms(engine, run, reps):
    torch.cuda.synchronize()  # the inputs, made on torch's stream (the runs go unordered on the engine's)
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    times = []
    for i in range(reps + 2):
        engine.signal_next(stop, start=start)
        run()
        stop.synchronize()
        if i >= 2:  # two warm-up runs
            times.append(start.elapsed_ms(stop))
    start.close()
    stop.close()
    return statistics.median(times)


def kernel_row(engine, name, streams, trials, reps):
    param = make_parameter(2, 4, 1024, 48000, False, trials)
    _, _, spb = LegacyCodec(engine.lib).block_size(1024, 2, 4)  # one block per stream
    pcm = (torch.randn((streams, spb, 2), device="cuda") * 6000).clamp(-32768, 32767).to(torch.int16)
    plan = engine.uniform_encode_plan(param, streams, spb)
    ref = torch.zeros((streams, plan.stride), dtype=torch.uint8, device="cuda")
    t_int = kernel_ms(engine, lambda: plan.run(pcm, ref, None, ordered=False), reps)
    planar_i16 = pcm.transpose(1, 2).contiguous()
    planar_f32 = planar_i16.float() / 32768
    d = plan.descs.copy()
    d["pcm_offset"] = np.arange(streams, dtype=np.uint64) * np.uint64(2 * spb)
    out = {}
    for dt, x in ((torch.int16, planar_i16), (torch.float32, planar_f32)):
        pp = engine.planar_encode_plan(param, d, spb, dt)
        got = torch.zeros_like(ref)
        t = kernel_ms(engine, lambda: pp.run(x, got, None, ordered=False), reps)
        torch.cuda.synchronize()
        exact = torch.equal(got, ref)
        pp.close()
        out[dt] = (t, exact)
    plan.close()
    ti, ei = out[torch.int16]
    tf, ef = out[torch.float32]
    return ("%-9s streams=%d trials=%d  interleaved %.4f ms  planar int16 %.4f ms (%.3fx, exact=%s)  planar float32 %.4f ms "
            "(%.3fx, exact=%s)" % (name, streams, trials, t_int, ti, ti / t_int, ei, tf, tf / t_int, ef))


def corpus_row(engine, streams, seconds):
    frames = 48000 * seconds
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    x = (torch.randn((streams, 2, frames), device="cuda") * 0.2).clamp_(-1, 1)
    torch.cuda.synchronize()

    def composite():
        pcm = torch.nan_to_num(x, nan=0.0).mul(32768).round().clamp(-32768, 32767).to(torch.int16).transpose(1, 2).contiguous()
        return engine.encode_uniform(pcm, param, segment_blocks=64, warmup_blocks=8)

    def planar():
        return engine.encode_planar(x, param, segment_blocks=64, warmup_blocks=8)

    res = {}
    for name, fn in (("composite", composite), ("planar", planar)):
        times, peak, out = [], 0, None
        for _ in range(3):
            out = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            images = out[0]
            peak = torch.cuda.max_memory_allocated() - base - images.numel()
        res[name] = (statistics.median(times), peak, out)
    (tc, pc, oc), (tp, pp_, op) = res["composite"], res["planar"]
    exact = oc[0].shape == op[0].shape and torch.equal(oc[0], op[0])
    return ("corpus    streams=%d x %d s stereo float32 (%.1f GB) L=64 W=8  composite %.1f ms, +%.2f GB  encode_planar %.1f ms (%.2fx "
            "faster), +%.3f GB above input + images  exact=%s" % (streams, seconds, x.numel() * 4 / 1e9, tc * 1e3, pc / 1e9, tp * 1e3,
                                                                    tc / tp, pp_ / 1e9, exact))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--corpus", action="store_true")
    ap.add_argument("--corpus-streams", type=int, default=1000)
    ap.add_argument("--corpus-seconds", type=int, default=60)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    engine = Engine(0)
    lines = []
    if not a.skip_kernels:
        for trials in (0, 2):
            lines.append(kernel_row(engine, "headline", 1000, trials, a.reps))
            print(lines[-1], flush=True)
        lines.append(kernel_row(engine, "saturated", 262144, 0, a.reps))
        print(lines[-1], flush=True)
    if a.corpus:
        lines.append(corpus_row(engine, a.corpus_streams, a.corpus_seconds))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    engine.close()


if __name__ == "__main__":
    main()
