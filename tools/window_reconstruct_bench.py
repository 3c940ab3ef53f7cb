"""Window reconstruct against the composite it replaces (profiles/r06_window_reconstruct.txt, DESIGN.md "Window reconstruct").

Corpus [--streams, 2, --seconds s] float32 on the device; N = 256 and N = 4096 windows of T = 48 000 frames drawn on the device;
4-bit, block 1024, float32 rows; unsegmented and segmented L = 8, W = 2.  Per row:
  window     Engine.reconstruct_windows: call time (wall, with a device synchronise, median of --call-reps), the run's own time
             from the events AADHip_ContextSignalNextRun puts around it (resolve kernel .. encoder kernel, median of --reps), peak
             device memory above the returned rows
  composite  INTEGRATION.md section 2g's former example: windows.tolist() twice, torch.stack of N slices, reconstruct_planar - call
             time, its parts (the two host copies, the gather, reconstruct_planar), the reconstruct kernel's own time, peak memory
  overhead   the window run's time minus the composite's reconstruct kernel's: what the resolve kernel and the gap between the
             run's launches cost on top of the same encoder launch (a difference of two medians).  The resolve kernel's OWN time is
             not visible to events around the run: take it from a kernel trace of this tool,
             `rocprofv3 --kernel-trace --stats -- python tools/window_reconstruct_bench.py --windows 4096 --reps 5 --call-reps 2`,
             row window_resolve_kernel.
Every row is bit-exact against the composite before a number is written: a row that is not prints why, nothing is appended to
--out and the tool exits with status 1.  Prints one line per row; --out appends them to a file."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aad_amd.capi import STREAM_DESC_DTYPE, make_parameter  # noqa: E402
from aad_amd.engine import Engine  # noqa: E402
from planar_reconstruct_bench import kernel_ms  # noqa: E402


def timed(fn, reps):
    """median wall time of fn() with a device synchronise, peak device memory above what fn's result keeps"""
    times, peak, out = [], 0, None
    for i in range(reps + 1):
        out = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i:  # one warm-up call
            times.append(time.perf_counter() - t0)
        peak = torch.cuda.max_memory_allocated() - before - out.numel() * out.element_size()
    return statistics.median(times), peak, out


def row(engine, corpus, n, frames, seg, reps, call_reps):
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    s, ch, total = corpus.shape
    kw = dict(segment_blocks=seg[0], warmup_blocks=seg[1]) if seg else {}
    g = torch.Generator(device="cuda").manual_seed(n)
    windows = torch.stack([torch.randint(0, s, (n,), device="cuda", generator=g),
                           torch.randint(0, total - frames + 1, (n,), device="cuda", generator=g)], dim=1)

    def gather():
        rows, first = windows[:, 0], windows[:, 1]
        return torch.stack([corpus[r, :, f:f + frames] for r, f in zip(rows.tolist(), first.tolist())])

    t_win, peak_win, y = timed(lambda: engine.reconstruct_windows(corpus, windows, frames, param, **kw), call_reps)
    t_comp, peak_comp, ref = timed(lambda: engine.reconstruct_planar(gather(), param, **kw), call_reps)
    exact = torch.equal(y.view(torch.int32), ref.view(torch.int32))
    t_sync, _, _ = timed(lambda: torch.tensor(windows[:, 0].tolist() + windows[:, 1].tolist()), call_reps)
    t_gather, _, x = timed(gather, call_reps)
    t_rec, _, _ = timed(lambda: engine.reconstruct_planar(x, param, **kw), call_reps)

    # the runs' own times, plans made once
    d = np.zeros(s, dtype=STREAM_DESC_DTYPE)
    d["pcm_offset"] = np.arange(s, dtype=np.uint64) * np.uint64(corpus.stride(0))
    d["num_samples"] = total
    wplan = engine.window_reconstruct_plan(param, d, corpus.stride(1), torch.float32, *(seg or (None, 0)))
    out = torch.empty((n, ch, frames), dtype=torch.float32, device="cuda")
    k_win = kernel_ms(engine, lambda: wplan.run(corpus, windows, frames, out=out, ordered=False), reps)
    exact = exact and torch.equal(out.view(torch.int32), ref.view(torch.int32))
    wplan.close()
    size = engine.encoded_size(param, frames)
    stride = (size + 63) // 64 * 64
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    d["pcm_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(ch * frames)
    d["data_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    d["data_size"], d["num_samples"] = stride, frames
    rplan = engine.planar_reconstruct_plan(param, d, frames, torch.float32, torch.float32, ch * frames, frames, *(seg or (None, 0)))
    images = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    k_rec = kernel_ms(engine, lambda: rplan.run(x, images, out, None, ordered=False), reps)
    rplan.close()
    if not exact:
        sys.exit("N=%d %s: NOT bit-exact against the composite - no number written" % (n, "L=%d W=%d" % seg if seg else "unsegmented"))
    mb = 1.0 / (1 << 20)
    return ("N=%-5d T=%d %-12s rows %.1f MiB  window: call %.3f ms, run %.3f ms, peak above rows %.1f MiB | composite: call %.3f ms "
            "(host copies %.3f, gather %.3f, reconstruct_planar %.3f; kernel %.3f ms), peak above rows %.1f MiB | call %.2fx | run minus "
            "kernel %.4f ms  exact=True" % (
                n, frames, "L=%d W=%d" % seg if seg else "unsegmented", y.numel() * 4 * mb, t_win * 1e3, k_win, peak_win * mb, t_comp * 1e3,
                t_sync * 1e3, t_gather * 1e3, t_rec * 1e3, k_rec, peak_comp * mb, t_comp / t_win, k_win - k_rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1000)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--windows", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--call-reps", type=int, default=25)
    ap.add_argument("--out")
    a = ap.parse_args()
    engine = Engine(0)
    corpus = torch.empty((a.streams, 2, 48000 * a.seconds), dtype=torch.float32, device="cuda")
    for i in range(0, a.streams, 50):  # in slices: randn's temporaries stay small
        corpus[i:i + 50] = (torch.randn((min(50, a.streams - i), 2, 48000 * a.seconds), device="cuda") * 0.2).clamp_(-1, 1)
    lines = ["corpus %s float32, 4-bit stereo, block 1024" % "x".join(str(v) for v in corpus.shape)]
    print(lines[0], flush=True)
    for n in a.windows:
        for seg in (None, (8, 2)):
            lines.append(row(engine, corpus, n, a.frames, seg, a.reps, a.call_reps))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    engine.close()


if __name__ == "__main__":
    main()
