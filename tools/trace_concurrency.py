#!/usr/bin/env python3
"""Kernel durations by how many other kernels ran beside them, and the kernel-to-kernel gaps of every queue, from a rocprofv3
--kernel-trace pass stored as a rocpd SQLite database.  bench.py runs its batch serially, with one step pipeline and with two
steps in flight: the "beside" column tells the three apart (0, 1 and 3 other kernels at work).
usage: tools/trace_concurrency.py <dir> [min calls per row]"""
import bisect
import collections
import glob
import os
import sqlite3
import statistics
import sys


def short(name):
    """template arguments are what tell the encoders apart: keep them, drop the argument list"""
    name = name.split("(")[0]
    return name if len(name) <= 96 else name[:93] + "..."


def main():
    root = sys.argv[1]
    min_calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    for db in sorted(glob.glob(os.path.join(root, "**", "*.db"), recursive=True)):
        con = sqlite3.connect(db)
        cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
        queue = next((c for c in ("queue_id", "stream_id", "queue", "stream") if c in cols), None)
        q = "select name, start, end, %s from kernels order by start" % (queue or "0")
        ks = [(n, s, e, qu) for n, s, e, qu in con.execute(q)]
        starts = [k[1] for k in ks]
        longest = max((k[2] - k[1] for k in ks), default=0)
        by = collections.defaultdict(list)
        beside_of = []
        for i, (n, s, e, qu) in enumerate(ks):
            # kernels that overlap at least half of this one
            lo = bisect.bisect_left(starts, s - longest)
            hi = bisect.bisect_right(starts, e)
            beside = 0
            for j in range(lo, hi):
                if j == i:
                    continue
                o = min(e, ks[j][2]) - max(s, ks[j][1])
                beside += 2 * o >= e - s
            beside_of.append(beside)
            by[(short(n), beside)].append(e - s)
        print("%s (queue column: %s)" % (os.path.basename(db), queue))
        print("%-100s %6s %6s %9s %9s %9s %9s" % ("kernel", "beside", "calls", "median us", "p10 us", "p90 us", "max us"))
        for (n, b), v in sorted(by.items(), key=lambda kv: (kv[0][0], kv[0][1])):
            if len(v) < min_calls:
                continue
            v.sort()
            print("%-100s %6d %6d %9.2f %9.2f %9.2f %9.2f" % (n, b, len(v), statistics.median(v) / 1e3, v[len(v) // 10] / 1e3,
                                                           v[len(v) * 9 // 10] / 1e3, v[-1] / 1e3))
        # gaps: from a kernel's end to the start of the next kernel of the same queue, where both ran beside the same count
        gaps = collections.defaultdict(list)
        prev = {}
        for i, (n, s, e, qu) in enumerate(ks):
            if qu in prev:
                pe, pb, pn = prev[qu]
                if pb == beside_of[i] and 0 <= s - pe < 50000:
                    gaps[(qu, short(pn) == short(n) and short(n) or "(mixed)", pb)].append(s - pe)
            prev[qu] = (e, beside_of[i], n)
        print("%-8s %-91s %6s %6s %9s %9s %9s" % ("queue", "kernel", "beside", "gaps", "median us", "p10 us", "p90 us"))
        for (qu, n, b), v in sorted(gaps.items(), key=lambda kv: (str(kv[0][0]), kv[0][1], kv[0][2])):
            if len(v) < min_calls:
                continue
            v.sort()
            print("%-8s %-91s %6d %6d %9.2f %9.2f %9.2f" % (qu, n, b, len(v), statistics.median(v) / 1e3, v[len(v) // 10] / 1e3,
                                                          v[len(v) * 9 // 10] / 1e3))


if __name__ == "__main__":
    main()
