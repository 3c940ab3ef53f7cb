#!/usr/bin/env python3
"""Count the issue slots of the quad encoder's chunk body in a gfx950 assembly listing (host only).

The listing comes from `hipcc --offload-arch=gfx950 -O3 --save-temps -c aad_amd/csrc/aad_hip_engine.hip`
(the `*-gfx950.s` file).  encode_chunk16_quad cuts every sample into two regions separated by
`sched_barrier`s, so a steady-state chunk is a run of barrier-delimited regions with no label or
branch inside.  The script finds the kernel by its template arguments, takes such a run in its main
loop, cuts it into samples at the quantiser's `v_fma_f32` (the only fma of the body) and prints every
sample's instructions - one slot each, s_nop and s_waitcnt included - with the per-sample counts and
the chunk's mean.  Sample 0 also carries whatever the loop issues in front of the chunk.

    tools/count_chunk_slots.py build.s                      # headline: 4-bit stereo quad, no trials
    tools/count_chunk_slots.py build.s --bits 3 --chf 1     # other instantiations
    tools/count_chunk_slots.py build.s --quiet              # counts only
"""
import argparse
import re
import sys

SAMPLES = 16


def kernel_symbol(bits, chf, ms, quad, trials, dual, ring):
    b = lambda v: "Lb1E" if v else "Lb0E"
    # <BITS, CHF, MS, QUAD, TRIALS, DUAL, RING, SEG = false, IN = interleaved, REC = none>; the argument type follows
    return "_ZN3aad21encode_streams_kernelILi%dELi%dE%s%s%s%s%sLb0ELi0ELi0EEEv" % (
        bits, chf, b(ms), b(quad), b(trials), b(dual), b(ring))


def kernel_lines(lines, sym):
    start = None
    for i, l in enumerate(lines):
        if l.startswith(sym) and re.match(r"^\w+:", l):
            start = i + 1
        elif start is not None and (l.startswith(".Lfunc_end") or re.match(r"^_Z\w*:", l)):
            return lines[start:i]
    if start is None:
        sys.exit("kernel %s not in the listing" % sym)
    return lines[start:]


def is_instruction(l):
    s = l.strip()
    return bool(s) and not s.startswith(";") and not s.startswith(".") and not s.endswith(":")


def chunk_runs(body):
    """Runs of sched_barrier-terminated regions with no label or branch inside, as instruction lists."""
    runs, cur, region, nreg = [], [], [], 0
    for l in body:
        s = l.strip()
        if "sched_barrier" in s:
            cur += region
            region = []
            nreg += 1
            continue
        if s.endswith(":") or s.startswith("s_cbranch") or s.startswith("s_branch"):
            if nreg >= 2 * SAMPLES:
                runs.append(cur)
            cur, region, nreg = [], [], 0
            continue
        if is_instruction(l):
            region.append(s.split(";")[0].strip())
    if nreg >= 2 * SAMPLES:
        runs.append(cur)
    return runs


def samples_of(run):
    """Cut a run at the quantisers: sample j = its fma up to the next sample's fma."""
    starts = [i for i, ins in enumerate(run) if ins.startswith("v_fma_f32")]
    if len(starts) < SAMPLES:
        return None
    out = []
    for j in range(SAMPLES):
        lo = 0 if j == 0 else starts[j]
        hi = starts[j + 1] if j + 1 < len(starts) else len(run)
        out.append(run[lo:hi])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("listing")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--chf", type=int, default=2)
    ap.add_argument("--ms", action="store_true")
    ap.add_argument("--trials", action="store_true")
    ap.add_argument("--dual", action="store_true")
    ap.add_argument("--run", type=int, default=0, help="which run of the kernel (default: the first)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args()
    lines = open(a.listing).read().splitlines()
    sym = kernel_symbol(a.bits, a.chf, a.ms, True, a.trials, a.dual, False)
    runs = [r for r in chunk_runs(kernel_lines(lines, sym)) if samples_of(r)]
    if len(runs) <= a.run:
        sys.exit("%s: %d chunk runs, --run %d asked for" % (sym, len(runs), a.run))
    samples = samples_of(runs[a.run])
    counts = [len(s) for s in samples]
    if not a.quiet:
        for j, s in enumerate(samples):
            print("sample %2d: %d slots" % (j, len(s)))
            for k, ins in enumerate(s):
                print("   %2d %s" % (k + 1, ins))
    flat = [i for s in samples for i in s]
    nops = sum(1 for i in flat if i.startswith("s_nop"))
    mem = sum(1 for i in flat if re.match(r"(global|buffer|flat)_", i))
    print("%s: %d runs; run %d: %d slots in %d samples = %.2f per sample (min %d, max %d; %d s_nop, %d global memory)"
          % (sym, len(runs), a.run, sum(counts), SAMPLES, sum(counts) / SAMPLES, min(counts), max(counts), nops, mem))


if __name__ == "__main__":
    main()
