"""Kernel time of segmented encode plans (AADHip_SegmentedEncodePlanCreate) against the serial plan, on the GPU.

Each case is one plan run, timed by the events AADHip_ContextSignalNextRun attaches to the run's own kernel dispatch (the kernel's
duration, no queue packets around it), median of --runs after --warmup untimed runs.  Cases (stereo 4-bit, 1024-byte blocks, fresh
encoders): one stream of 2000 blocks; 16 such streams; 1000 one-block streams (the control: one chain per stream whatever L and W
are, so a segmented plan must time like the serial one).  Each against serial and (L, W) in {(16,4), (64,8), (128,16), (256,32)},
at 0 and 2 trials.  The tool only times: the bytes are tests/test_gpu_segmented_encode.py's business.

    python tools/segmented_encode_probe.py [--runs 20] [--warmup 3] [--out profiles/r05_segmented_encode.txt]

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
CASES = [("1 x 2000 blocks", 1, 2000), ("16 x 2000 blocks", 16, 2000), ("1000 x 1 block (control)", 1000, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_segmented_encode.txt"))
    args = ap.parse_args()
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
