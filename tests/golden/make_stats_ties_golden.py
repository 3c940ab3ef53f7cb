#!/usr/bin/env python3
"""Streams whose `aad -c` statistics lie on a rounding boundary of the printed six decimals (tests/golden/stats_ties.json).

compare_finish_kernel (aad_amd/csrc/aad_compare.hip.h) sums in a tree and re-sums a stream in the reference's order only when
its RMSE or MSD lies within rel(n) = compare_reorder_bound(n) of a boundary (k + 1/2) 1e-6 (aad_compare_round.h).  Random
streams land there about once in 10^5, so the suite's other inputs never take that branch.  This script finds inputs that do.

Search: at trials = 0 the reconstruction of a prefix x[:m] of a synth stream is the first m frames of the reconstruction of x
(the encoder looks only backwards; every kept case is re-encoded whole below, so nothing rests on that).  One oracle encode and
decode of x gives e for every value (the reference's formula, src/main.c:478-491, in numpy: each e is exact).  Mono: the
reference's order is a running sum, so np.cumsum scores every prefix length at once.  More channels: the channel-major order
of a prefix is not a prefix of anything, so the per-channel running sums pick candidates (within 6 windows), which are then
summed in the reference's order by the oracle.  Kept: oracle RMSE or MSD within 1/4 of the kernel's window of a boundary
(tie), or between 1.5 and 4 windows from one (control: the kernel must NOT re-sum).

Runs only in the build container: it executes oracle/_ref/aad, the reference CLI compiled by oracle/Makefile, on the WAV of
every case and keeps the line it prints.  Data only: the recipe, the oracle's three doubles (float.hex) and that line.
"""
import json
import os
import subprocess
import sys
import tempfile
import time
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_binding as ob  # noqa: E402
from aad_amd.synth import synth_pcm  # noqa: E402
from helpers import wav16_bytes  # noqa: E402

CLI = os.path.join(ROOT, "oracle", "_ref", "aad")
INT32_MAX = 2147483647.0
BLOCK = 1024

# (kind, seed, channels, frames searched, bits, M/S, statistic of the one control kept or None): at most 2M values per stream.
# Mono and stereo only: the reference CLI takes no more channels.
SEARCHES = [("noise", 11, 1, 2_000_000, 2, False, "rmse"), ("music", 11, 1, 2_000_000, 4, False, None),
            ("noise", 12, 2, 1_000_000, 3, False, "msd"), ("music", 13, 2, 1_000_000, 4, True, "rmse")]
# ties kept per statistic and search: the shortest of at least 1000 frames, and the shortest beyond 1/8 of the search


def rel(n):
    """compare_reorder_bound (aad_compare_round.h), the same double"""
    return 2.5 * float(n) * 1.1102230246251565e-16 + 1e-15


def distance_in_windows(v, n):
    """|v - nearest boundary| / (v rel(n)), exact"""
    q = Fraction(v) * 10 ** 6
    k = (q - Fraction(1, 2)).__round__()
    return float(abs(q - (k + Fraction(1, 2))) / (q * Fraction(rel(n))))


def errors(x, y):
    """e per value, [frames, channels], the reference's formula"""
    gap = ((x.astype(np.int64) << 16) - (y.astype(np.int64) << 16)).astype(np.int32)  # the 32-bit wrap, src/main.c:470-474
    return gap / INT32_MAX - y.astype(np.float64) / INT32_MAX


def candidates(e):
    """prefix lengths m (frames) with an estimate of (RMSE, MSD) each"""
    frames, ch = e.shape
    m = np.arange(1, frames + 1, dtype=np.float64)
    sq = np.cumsum(e * e, axis=0).sum(axis=1)
    ab = np.cumsum(np.abs(e), axis=0).sum(axis=1)
    return np.sqrt(sq / (ch * m)), ab / (ch * m)


def near(v, n, windows):
    """boolean mask: v within `windows` of the kernel's window of a boundary"""
    q = v * 1e6
    d = np.abs(q - (np.floor(q) + 0.5))
    return d <= windows * q * (2.5 * n * 1.1102230246251565e-16 + 1e-15)


def main():
    t_start = time.time()
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        for kind, seed, ch, frames, bits, ms, control in SEARCHES:
            t0 = time.time()
            x = synth_pcm(1, frames, ch, seed=seed, kind=kind)[0]
            y = ob.decode(ob.encode(x, bits, BLOCK, 48000, ms, 0))[0]
            e = errors(x, y)
            rms, msd = candidates(e)
            n = np.arange(1, frames + 1, dtype=np.float64) * ch
            found = {}
            for stat, est in (("rmse", rms), ("msd", msd)):
                # mono: the estimate IS the reference's order; otherwise it is within ~n u of it, about one window
                pick = np.nonzero(near(est, n, 4.0 if ch == 1 else 6.0))[0] + 1
                slots = [("tie", 1000, frames // 8), ("tie", frames // 8, frames + 1)] + ([("control", 1000, frames + 1)] if stat == control else [])
                for tag, lo, hi in slots:
                    for m in pick[(pick >= lo) & (pick < hi)]:
                        m = int(m)
                        st = ob.error_stats(x[:m], y[:m])
                        w = distance_in_windows(st[0 if stat == "rmse" else 1], m * ch)
                        if (w <= 0.25) if tag == "tie" else (1.5 <= w <= 4):
                            found.setdefault((stat, tag), []).append((m, st, w))
                            break
            for (stat, tag), kept in found.items():
                for m, st, w in kept:
                    xp = x[:m]
                    yp = ob.decode(ob.encode(xp, bits, BLOCK, 48000, ms, 0))[0]  # the prefix, whole
                    assert np.array_equal(yp, y[:m]), (kind, seed, ch, m)
                    assert ob.error_stats(xp, yp) == st
                    wav = os.path.join(tmp, "in.wav")
                    open(wav, "wb").write(wav16_bytes(xp, 48000))
                    opts = ["-b", str(bits), "-s", str(BLOCK), "-t", "0"] + (["-m"] if ms else [])
                    line = subprocess.run([CLI, "-c"] + opts + [wav], check=True, capture_output=True, text=True).stdout
                    assert line == ob.stats_line(st), (line, st)
                    cases.append(dict(kind=kind, seed=seed, channels=ch, frames=m, bits=bits, block_size=BLOCK, ms=ms, trials=0,
                                      statistic=stat, tie=tag == "tie", windows=round(w, 4),
                                      stats_hex=[float(v).hex() for v in st], stats_line=line))
            print("%s seed %d, %d ch, %d frames, %d-bit%s: %s (%.1f s)" % (
                kind, seed, ch, frames, bits, " M/S" if ms else "",
                ", ".join("%s %s %d" % (s, t, len(v)) for (s, t), v in found.items()), time.time() - t0))
    elapsed = time.time() - t_start
    with open(os.path.join(HERE, "stats_ties.json"), "w") as f:
        json.dump(dict(generator="tests/golden/make_stats_ties_golden.py", search_seconds=round(elapsed, 1), cases=cases), f, indent=1)
    print("stats tie cases:", sum(c["tie"] for c in cases), "controls:", sum(not c["tie"] for c in cases), "%.1f s" % elapsed)


if __name__ == "__main__":
    main()
