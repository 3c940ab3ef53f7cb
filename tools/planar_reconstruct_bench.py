"""Planar reconstruct against its two-kernel composite (profiles/r05_planar_reconstruct.txt, DESIGN.md "Planar reconstruct").

Kernel rows: each kernel's own time from the events AADHip_ContextSignalNextRun attaches to its dispatch, median of --reps runs.
The fused kernel (AADHip_PlanarReconstructPlanRun, float32 [N, C, T] in and out) against the planar encode kernel alone
(AADHip_PlanarEncodePlanRun) and against planar encode + window decode (AADHip_WindowDecodePlanRun with windows (i, 0), float32
rows) - the route the fused form replaces.  Every row checks the fused run bit for bit: images equal to the planar encode's,
rows equal to the window decode's.
  headline   1000 stereo 4-bit one-block streams, t = 0 (bench.py's shape)
  saturated  262 144 such streams
  trials     the headline shape with t = 2: the composite's encode takes the dual trial search, the fused kernel the single one
Corpus row (--corpus): 1000 stereo 60 s streams at 48 kHz as float32 [N, C, T], segmented L = 64, W = 8 - Engine.reconstruct_planar
against Engine.encode_planar + Engine.decode_windows over the whole streams: wall time of the call (median of three, synchronised).
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
from aad_amd.engine import Engine, HipEvent, parse_header  # noqa: E402


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
    x = ((torch.randn((streams, 2, spb), device="cuda") * 6000).clamp(-32768, 32767).round() / 32768).contiguous()
    size = engine.encoded_size(param, spb)
    stride = (size + 63) // 64 * 64
    d = np.zeros(streams, dtype=[("pcm_offset", "<u8"), ("data_offset", "<u8"), ("data_size", "<u8"), ("num_samples", "<u4"),
                                 ("reserved", "<u4")])
    d["pcm_offset"] = np.arange(streams, dtype=np.uint64) * np.uint64(2 * spb)
    d["data_offset"] = np.arange(streams, dtype=np.uint64) * np.uint64(stride)
    d["data_size"] = stride
    d["num_samples"] = spb
    enc = engine.planar_encode_plan(param, d, spb, torch.float32)
    ref = torch.zeros((streams, stride), dtype=torch.uint8, device="cuda")
    t_enc = kernel_ms(engine, lambda: enc.run(x, ref, None, ordered=False), reps)
    torch.cuda.synchronize()
    wd = d.copy()
    wd["data_size"] = size
    win = engine.window_decode_plan(parse_header(bytes(ref[0, :31].cpu().numpy())), wd, True)
    windows = torch.zeros((streams, 2), dtype=torch.int64, device="cuda")
    windows[:, 0] = torch.arange(streams, device="cuda")
    yref = torch.zeros((streams, 2, spb), dtype=torch.float32, device="cuda")
    t_dec = kernel_ms(engine, lambda: win.run(ref, windows, spb, torch.float32, yref, ordered=False), reps)
    rec = engine.planar_reconstruct_plan(param, d, spb, torch.float32, torch.float32, 2 * spb, spb)
    img = torch.zeros_like(ref)
    y = torch.zeros_like(yref)
    t_rec = kernel_ms(engine, lambda: rec.run(x, img, y, None, ordered=False), reps)
    torch.cuda.synchronize()
    exact = torch.equal(img, ref) and torch.equal(y.view(torch.int32), yref.view(torch.int32))
    for p in (enc, win, rec):
        p.close()
    return ("%-9s streams=%d trials=%d float32 in/out  fused %.4f ms  planar encode %.4f ms (fused %.3fx)  window decode %.4f ms  "
            "encode + decode %.4f ms (fused %.3fx)  exact=%s" % (name, streams, trials, t_rec, t_enc, t_rec / t_enc, t_dec,
                                                                 t_enc + t_dec, t_rec / (t_enc + t_dec), exact))


def corpus_row(engine, streams, seconds):
    frames = 48000 * seconds
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    x = (torch.randn((streams, 2, frames), device="cuda") * 0.2).clamp_(-1, 1)
    windows = torch.zeros((streams, 2), dtype=torch.int64, device="cuda")
    windows[:, 0] = torch.arange(streams, device="cuda")
    torch.cuda.synchronize()

    def composite():
        images, sizes = engine.encode_planar(x, param, segment_blocks=64, warmup_blocks=8)
        return engine.decode_windows(images, max(sizes), windows, frames), images

    def fused():
        y, images, _ = engine.reconstruct_planar(x, param, segment_blocks=64, warmup_blocks=8, return_images=True)
        return y, images

    res = {}
    for name, fn in (("composite", composite), ("fused", fused)):
        times, out = [], None
        for _ in range(3):
            out = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res[name] = (statistics.median(times), out)
    (tc, oc), (tf, of) = res["composite"], res["fused"]
    exact = torch.equal(oc[1], of[1]) and torch.equal(oc[0].view(torch.int32), of[0].view(torch.int32))
    return ("corpus    streams=%d x %d s stereo float32 (%.1f GB) L=64 W=8  encode_planar + decode_windows %.1f ms  reconstruct_planar "
            "%.1f ms (%.3fx)  exact=%s" % (streams, seconds, x.numel() * 4 / 1e9, tc * 1e3, tf * 1e3, tf / tc, exact))


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
        for name, streams, trials in (("headline", 1000, 0), ("saturated", 262144, 0), ("trials", 1000, 2)):
            lines.append(kernel_row(engine, name, streams, trials, a.reps))
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
