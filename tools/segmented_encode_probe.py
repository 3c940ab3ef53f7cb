"""Kernel time of segmented encode plans (AADHip_SegmentedEncodePlanCreate) against the serial plan, on the GPU.

Each case is one plan run, timed by the events AADHip_ContextSignalNextRun attaches to the run's own kernel dispatch (the kernel's
duration, no queue packets around it), median of --runs after --warmup untimed runs.  Cases (stereo 4-bit, 1024-byte blocks, fresh
encoders): one stream of 2000 blocks; 16 such streams; 1000 one-block streams (the control: one chain per stream whatever L and W
are, so a segmented plan must time like the serial one).  Each against serial and (L, W) in {(16,4), (64,8), (128,16), (256,32)},
at 0 and 2 trials.  The tool only times: the bytes are tests/test_gpu_segmented_encode.py's business.

    python tools/segmented_encode_probe.py [--runs 20] [--warmup 3] [--out profiles/r05_segmented_encode.txt]
    python tools/segmented_encode_probe.py --host [--runs 5] [--warmup 1] [--out profiles/r05_segmented_host.txt]

--host times the host-memory entry points instead, on the wall clock of the calling thread (PCIe and staging included): one stream of
2000 blocks (one staging chunk) and one 10-minute stream (29 032 blocks, ~130 MB up in 16 MiB chunks, one launch; at most 3 runs) through
AADHip_EncodeBatch (serial) against AADHip_SegmentedEncodeBatch at (16,4), (64,8) and (256,32), at 0 and 2 trials;
then `aad_batch -e` on one 10-minute stereo WAV, default against `-S 256,32` (-t 2, the CLI's default), and the `-c` line of both.

Clock caveat (measuring guide): the MI355X runs its clocks by load and power; a one-stream kernel of 100+ ms and a 1000-stream
kernel of 60 us see different clocks, and other work on the host's other GPUs can move either.  Compare cases within one run of the
tool, not across runs."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENTATIONS = [None, (16, 4), (64, 8), (128, 16), (256, 32)]
HOST_SEGMENTATIONS = [None, (16, 4), (64, 8), (256, 32)]
CASES = [("1 x 2000 blocks", 1, 2000), ("16 x 2000 blocks", 16, 2000), ("1000 x 1 block (control)", 1000, 1)]


def host_rows(args):
    """AADHip_EncodeBatch against AADHip_SegmentedEncodeBatch, host buffers in and out, wall clock per call"""
    import numpy as np
    import torch
    from aad_amd.engine import Engine
    from aad_amd.synth import synth_pcm
    eng = Engine(0)
    lines = ["# segmented encode from host memory: wall time of one call on the calling thread (median of %d after %d warm-up)"
             % (args.runs, args.warmup),
             "# stereo 4-bit, max block size 1024 (992 samples per block), one stream, music-like synthetic input",
             "# device: %s" % torch.cuda.get_device_name(0),
             "%-22s %-30s %6s %-10s %10s %10s %10s %9s" % ("stream", "entry point", "trials", "L,W", "median_ms", "min_ms", "max_ms", "speedup")]
    print("\n".join(lines), flush=True)
    for name, frames, runs in (("2000 blocks", 2000 * 992, args.runs), ("10 min (29032 blocks)", 600 * 48000, min(args.runs, 3))):
        lines += host_case(args, eng, name, np.ascontiguousarray(synth_pcm(1, frames, 2, seed=7)[0]), runs)
    eng.close()
    return lines


def host_case(args, eng, name, pcm, runs):
    import ctypes as C
    import time
    import numpy as np
    from aad_amd.capi import AADHipSegmentation, make_parameter
    lines = []
    for trials in (0, 2):
        param = make_parameter(2, 4, 1024, 48000, False, trials)
        size = eng.encoded_size(param, pcm.shape[0])
        out = np.zeros(size, dtype=np.uint8)
        n = (C.c_uint32 * 1)(pcm.shape[0])
        pp, op = (C.c_void_p * 1)(pcm.ctypes.data), (C.c_void_p * 1)(out.ctypes.data)
        cap, got = (C.c_uint64 * 1)(size), (C.c_uint64 * 1)(0)
        serial_ms = None
        for seg in HOST_SEGMENTATIONS:
            if seg is None:
                call = lambda: eng.lib.AADHip_EncodeBatch(eng._ctx, C.byref(param), 1, pp, n, op, cap, got, None)
            else:
                s = AADHipSegmentation(*seg)
                call = lambda s=s: eng.lib.AADHip_SegmentedEncodeBatch(eng._ctx, C.byref(param), C.byref(s), 1, pp, n, op, cap, got)
            times = []
            for k in range(args.warmup + runs):
                t0 = time.perf_counter()
                rc = call()
                t1 = time.perf_counter()
                assert rc == 0, rc
                if k >= args.warmup:
                    times.append((t1 - t0) * 1e3)
            med = statistics.median(times)
            if seg is None:
                serial_ms = med
            row = "%-22s %-30s %6d %-10s %10.3f %10.3f %10.3f %9s" % (
                name, "AADHip_EncodeBatch" if seg is None else "AADHip_SegmentedEncodeBatch", trials,
                "serial" if seg is None else "%d,%d" % seg, med, min(times), max(times), "%.2fx" % (serial_ms / med))
            print(row, flush=True)
            lines.append(row)
    return lines


def cli_rows():
    """aad_batch -e / -c on one 10-minute stereo WAV, default against -S 256,32"""
    import subprocess
    import tempfile
    import time
    from aad_amd.synth import synth_pcm
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import wav16_bytes
    cli = os.path.join(ROOT, "aad_amd", "aad_batch")
    lines = ["", "# aad_batch on one 10-minute stereo WAV (48 kHz, 28.8 M frames), CLI defaults (-b 4 -s 1024 -t 2): wall time of the process"]
    print(lines[-1], flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "ten_minutes.wav")
        with open(wav, "wb") as f:
            f.write(wav16_bytes(synth_pcm(1, 600 * 48000, 2, seed=3)[0], 48000))
        for opts in ([], ["-S", "256,32"]):
            out = os.path.join(tmp, "out%d" % len(opts))
            os.mkdir(out)
            t0 = time.perf_counter()
            subprocess.run([cli, "-e", "-o", out] + opts + [wav], check=True, timeout=600)
            t1 = time.perf_counter()
            c = subprocess.run([cli, "-c"] + opts + [wav], check=True, timeout=600, capture_output=True, text=True).stdout
            row = "%-14s -e %8.3f s   -c: %s" % (" ".join(opts) or "default", t1 - t0, c.split("\t", 1)[1].rstrip())
            print(row, flush=True)
            lines.append(row)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host", action="store_true", help="the host-memory entry points and aad_batch (see above)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.host:
        lines = host_rows(args) + cli_rows()
        out = args.out or os.path.join(ROOT, "profiles", "r05_segmented_host.txt")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "r05_segmented_encode.txt")
    import torch
    from aad_amd.capi import make_parameter
    from aad_amd.engine import Engine, HipEvent
    from aad_amd.synth import synth_pcm
    assert torch.cuda.is_available(), "the probe times kernels: it needs the GPU"

    eng = Engine(0)
    lines = ["# segmented encode: kernel time of one AADHip_EncodePlanRun (events on the dispatch, median of %d runs after %d warm-up)"
             % (args.runs, args.warmup),
             "# stereo 4-bit, max block size 1024 (992 samples per block), music-like synthetic input, mapping auto, trial lanes dual",
             "# device: %s" % torch.cuda.get_device_name(0),
             "# clocks follow load and power: compare rows of one run, not across runs",
             "%-26s %6s %-10s %7s %10s %10s %10s %9s" % ("case", "trials", "L,W", "chains", "median_ms", "min_ms", "max_ms", "speedup")]
    print("\n".join(lines), flush=True)
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    for trials in (0, 2):
        param = make_parameter(2, 4, 1024, 48000, False, trials)
        for name, streams, blocks in CASES:
            samples = blocks * 992
            pcm = torch.from_numpy(synth_pcm(streams, samples, 2, seed=7)).cuda()
            serial_ms = None
            for seg in SEGMENTATIONS:
                L, W = seg if seg else (None, 0)
                plan = eng.uniform_encode_plan(param, streams, samples, L, W)
                out = torch.zeros((streams, plan.stride), dtype=torch.uint8, device="cuda")
                for _ in range(args.warmup):
                    plan.run(pcm, out)
                torch.cuda.synchronize()
                times = []
                for _ in range(args.runs):
                    eng.signal_next(stop, start=start)
                    plan.run(pcm, out)
                    stop.synchronize()
                    times.append(start.elapsed_ms(stop))
                plan.close()
                med = statistics.median(times)
                if seg is None:
                    serial_ms = med
                chains = streams * (-(-blocks // L) if L else 1)
                row = "%-26s %6d %-10s %7d %10.4f %10.4f %10.4f %9s" % (
                    name, trials, "serial" if seg is None else "%d,%d" % seg, chains, med, min(times), max(times),
                    "%.2fx" % (serial_ms / med))
                print(row, flush=True)
                lines.append(row)
    eng.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
