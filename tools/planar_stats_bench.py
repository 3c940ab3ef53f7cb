"""Planar reconstruct statistics against the plain reconstruct kernel and against the torch composite they replace
(profiles/r05_planar_stats.txt, DESIGN.md "Planar reconstruct statistics").

Kernel rows: each kernel's own time from the events AADHip_ContextSignalNextRun attaches to its dispatch, median of --reps runs.
The statistics kernel (AADHip_PlanarReconstructPlanRunStats, float32 [N, C, T] in and out), its rows-free form (device_out = NULL)
and the plain reconstruct kernel of the same build (AADHip_PlanarReconstructPlanRun).  Every row checks images and rows bit for
bit against the plain run, and the records against torch int64 arithmetic on the plain run's rows.
  headline   1000 stereo 4-bit one-block streams, t = 0 (bench.py's shape)
  trials     the same with t = 2
  saturated  262 144 such streams
Call rows: Engine.reconstruct_planar(return_stats=True) and Engine.codec_error against what a user writes without them -
reconstruct_planar, then re-quantise the input, widen both to int64, subtract, square and reduce three times - as wall time of the
call with a device synchronise (median of --call-reps) and peak device memory above what is allocated before the call
(torch.cuda.max_memory_allocated), on the headline shape and, with --corpus, on 1000 stereo 60 s streams segmented L = 64, W = 8.
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

from aad_amd.capi import STREAM_DESC_DTYPE, LegacyCodec, make_parameter  # noqa: E402
from aad_amd.engine import Engine  # noqa: E402
from planar_reconstruct_bench import kernel_ms  # noqa: E402


def torch_stats(x, y):
    """the composite: q(x) - y * 32768 in int64 and its three reductions -> int64 [N, C, 4]"""
    e = torch.nan_to_num(x, nan=0.0).mul(32768.0).round().clamp(-32768, 32767).to(torch.int64)
    e -= y.mul(32768.0).to(torch.int64)  # in place: the corpus shape's int64 temporaries are 46 GB each
    a = e.abs()
    return torch.stack([(e * e).sum(-1), a.sum(-1), a.amax(-1), torch.full_like(a[..., 0], x.shape[-1])], dim=-1)


def kernel_row(engine, name, streams, trials, reps):
    param = make_parameter(2, 4, 1024, 48000, False, trials)
    _, _, spb = LegacyCodec(engine.lib).block_size(1024, 2, 4)  # one block per stream
    x = ((torch.randn((streams, 2, spb), device="cuda") * 6000).clamp(-32768, 32767).round() / 32768).contiguous()
    size = engine.encoded_size(param, spb)
    stride = (size + 63) // 64 * 64
    d = np.zeros(streams, dtype=STREAM_DESC_DTYPE)
    d["pcm_offset"] = np.arange(streams, dtype=np.uint64) * np.uint64(2 * spb)
    d["data_offset"] = np.arange(streams, dtype=np.uint64) * np.uint64(stride)
    d["data_size"] = stride
    d["num_samples"] = spb
    rec = engine.planar_reconstruct_plan(param, d, spb, torch.float32, torch.float32, 2 * spb, spb)
    ref = torch.zeros((streams, stride), dtype=torch.uint8, device="cuda")
    yref = torch.zeros((streams, 2, spb), dtype=torch.float32, device="cuda")
    img, y = torch.zeros_like(ref), torch.zeros_like(yref)
    img2 = torch.zeros_like(ref)
    stats = torch.full((streams, 2, 4), -1, dtype=torch.int64, device="cuda")
    only = torch.full((streams, 2, 4), -1, dtype=torch.int64, device="cuda")
    t_plain = kernel_ms(engine, lambda: rec.run(x, ref, yref, None, ordered=False), reps)
    t_stats = kernel_ms(engine, lambda: rec.run(x, img, y, None, ordered=False, stats=stats), reps)
    t_only = kernel_ms(engine, lambda: rec.run(x, img2, None, None, ordered=False, stats=only), reps)
    t_plain2 = kernel_ms(engine, lambda: rec.run(x, ref, yref, None, ordered=False), reps)  # again: drift between the first and the last
    torch.cuda.synchronize()
    exact = (torch.equal(img, ref) and torch.equal(img2, ref) and torch.equal(y.view(torch.int32), yref.view(torch.int32))
             and torch.equal(stats, torch_stats(x, yref)) and torch.equal(only, stats))
    rec.close()
    return ("%-9s streams=%d trials=%d float32 in/out  plain %.4f ms (again %.4f)  with statistics %.4f ms (%.3fx)  statistics only "
            "%.4f ms (%.3fx)  exact=%s" % (name, streams, trials, t_plain, t_plain2, t_stats, t_stats / t_plain, t_only,
                                           t_only / t_plain, exact))


def call_row(engine, name, x, reps, **kw):
    param = make_parameter(2, 4, 1024, 48000, False, 0)

    def composite():
        y = engine.reconstruct_planar(x, param, **kw)
        return y, torch_stats(x, y)

    def fused():
        return engine.reconstruct_planar(x, param, return_stats=True, **kw)

    def error_only():
        return None, engine.codec_error(x, param, **kw)

    res = {}
    for what, fn in (("composite", composite), ("fused", fused), ("codec_error", error_only)):
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
            peak = torch.cuda.max_memory_allocated() - before
        kept = sum(t.numel() * t.element_size() for t in out if t is not None)
        res[what] = (statistics.median(times), peak, kept, out)
    (tc, pc, kc, oc), (tf, pf, kf, of), (te, pe, ke, oe) = res["composite"], res["fused"], res["codec_error"]
    exact = torch.equal(oc[0].view(torch.int32), of[0].view(torch.int32)) and torch.equal(oc[1], of[1]) and torch.equal(oc[1], oe[1])
    mb = 1.0 / (1 << 20)
    return ("%-9s %s float32 %s  composite %.3f ms, peak %.1f MiB for %.1f MiB of results  return_stats %.3f ms (%.3fx), peak %.1f MiB "
            "for %.1f MiB (images %.1f MiB inside the call)  codec_error %.3f ms (%.3fx), peak %.1f MiB  exact=%s" % (
                name, "x".join(str(v) for v in x.shape), " ".join("%s=%s" % kv for kv in kw.items()), tc * 1e3, pc * mb, kc * mb,
                tf * 1e3, tf / tc, pf * mb, kf * mb, (pf - kf) * mb, te * 1e3, te / tc, pe * mb, exact))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--call-reps", type=int, default=9)
    ap.add_argument("--corpus", action="store_true")
    ap.add_argument("--corpus-streams", type=int, default=1000)
    ap.add_argument("--corpus-seconds", type=int, default=60)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    engine = Engine(0)
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    if not a.skip_kernels:
        for name, streams, trials in (("headline", 1000, 0), ("trials", 1000, 2), ("saturated", 262144, 0)):
            emit(kernel_row(engine, name, streams, trials, a.reps))
    _, _, spb = LegacyCodec(engine.lib).block_size(1024, 2, 4)
    emit(call_row(engine, "headline", (torch.randn((1000, 2, spb), device="cuda") * 0.2).clamp_(-1, 1), a.call_reps))
    if a.corpus:
        x = (torch.randn((a.corpus_streams, 2, 48000 * a.corpus_seconds), device="cuda") * 0.2).clamp_(-1, 1)
        emit(call_row(engine, "corpus", x, 3, segment_blocks=64, warmup_blocks=8))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    engine.close()


if __name__ == "__main__":
    main()
