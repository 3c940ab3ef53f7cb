#!/usr/bin/env python3
"""Which kernels tests/test_gpu_encode_matrix.py really launches, from a kernel trace, against the reachable records of
tests/encode_matrix.py.  One confirmation run on a GPU, not a test: the matrix file itself asserts the plan of every launch
(aad_launch_policy.h); this reads the names the runtime dispatched.

    python tools/kernel_trace_census.py [--out DIR] [--trace FILE.csv ...]

Runs `rocprofv3 --kernel-trace -M -f csv -d DIR -o trace -- python -m pytest tests/test_gpu_encode_matrix.py` - a kernel trace
alone, no counters and no other tracing in the same run; -M keeps the mangled names, which tests/kernel_names.py parses as it
parses the library's - and prints the two differences between "launched" and "the table's records".  --trace reads trace files of
an earlier run instead.  Exit status 0: both differences are empty and the test run passed."""
import argparse
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import encode_matrix as em  # noqa: E402
import kernel_names  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "kernel_trace_census"), help="directory for the trace")
    ap.add_argument("--trace", nargs="*", help="kernel trace CSV files of an earlier run (skips the run)")
    args = ap.parse_args()
    rc = 0
    traces = args.trace
    if not traces:
        cmd = ["rocprofv3", "--kernel-trace", "-M", "-f", "csv", "-d", args.out, "-o", "trace", "--", sys.executable, "-m", "pytest",
               os.path.join("tests", em.GPU_FILE), "-q", "-p", "no:cacheprovider"]
        print("+", " ".join(cmd), flush=True)
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        traces = sorted(glob.glob(os.path.join(args.out, "**", "*kernel_trace.csv"), recursive=True))
    if not traces:
        print("no kernel trace was written under", args.out)
        return 2
    data = b""
    for path in traces:
        with open(path, "rb") as f:
            data += f.read()
    table = {(c.kernel, c.args) for c in em.matrix_cells()}
    families = {k for k, _ in table}
    every = kernel_names.kernels_in(data)
    launched = {k for k in every if k[0] in families}
    others = sorted({k[0] for k in every} - families)
    stray, silent = sorted(launched - table), sorted(table - launched)
    print("trace files:", len(traces), "dispatch records:", max(data.count(b"\n") - len(traces), 0))
    for family in sorted(families):
        print("%-24s launched %4d of %4d records" % (family, sum(k[0] == family for k in launched), sum(k[0] == family for k in table)))
    print("launched and not a record of the table (%d):" % len(stray), stray)
    print("a record of the table and not launched (%d):" % len(silent), silent)
    print("other kernels of namespace aad in the trace:", others)
    print("test run exit status:", rc)
    return 1 if stray or silent or rc else 0


if __name__ == "__main__":
    sys.exit(main())
