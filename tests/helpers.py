"""Shared test helpers: minimal RIFF/WAVE PCM16 reader/writer and hashing."""
import hashlib
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def sha256(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def read_wav16(path):
    """-> (int16 [samples, channels], rate).  Skips unknown chunks like the reference reader
    (src/wav.c:176-193); only 16-bit PCM is needed for the fixtures."""
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(b):
        cid, size = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        body = b[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            data = body
            break
        pos += 8 + size + (size & 1)
    tag, ch, rate, _, _, bits = fmt
    assert tag == 1 and bits == 16
    x = np.frombuffer(data, dtype="<i2")
    return x[: len(x) // ch * ch].reshape(-1, ch).copy(), rate


def wav16_bytes(pcm, rate):
    """Canonical 44-byte-header WAV image, the layout the reference writer emits
    (src/wav.c:545-627) for 16-bit PCM."""
    pcm = np.ascontiguousarray(pcm, dtype="<i2")
    n, ch = pcm.shape
    payload = pcm.tobytes()
    head = b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, 1, ch, rate, rate * 2 * ch, 2 * ch, 16) + b"data" + struct.pack("<I", len(payload))
    return head + payload


def cli_mode_input(case):
    """Rebuild the WAV input of a tests/golden/cli_modes.json case -> (pcm int16 [n, ch], rate, wav bytes)."""
    import os as _os
    src = case["source"]
    if "fixture" in src:
        path = _os.path.join(GOLDEN, "ref_fixtures", src["fixture"])
        pcm, rate = read_wav16(path)
        data = open(path, "rb").read()
    else:
        from aad_amd.synth import synth_pcm
        pcm, rate = synth_pcm(1, src["samples"], src["channels"], seed=src["seed"], kind=src["kind"])[0], 48000
        data = wav16_bytes(pcm, rate)
    assert sha256(data) == case["input_sha256"]
    return pcm, rate, data


def wav_bytes_depth(pcm, rate, depth, salt=0):
    """A PCM WAV image of `depth` bits per sample (8 / 16 / 24 / 32) whose top 16 bits per sample are
    `pcm` (int16 [samples, channels]) - 8-bit keeps only the top byte - and whose lower bits are
    deterministic filler (an LCG seeded by `salt`), so that a reader which does not discard them by
    the reference's rule (src/main.c:175-179, src/wav.c:392-417) gives different codes."""
    pcm = np.ascontiguousarray(pcm, dtype="<i2")
    n, ch = pcm.shape
    flat = pcm.reshape(-1).astype(np.int64)
    x = (np.arange(flat.size, dtype=np.uint64) * np.uint64(6364136223846793005) + np.uint64(1442695040888963407 + salt))
    low = ((x >> np.uint64(40)) & np.uint64(0xFFFF)).astype(np.int64)
    if depth == 8:
        payload = (((flat >> 8) + 128) & 0xFF).astype(np.uint8).tobytes()
    elif depth == 16:
        payload = pcm.tobytes()
    elif depth == 24:
        v = ((flat << 8) | (low & 0xFF)) & 0xFFFFFF
        b = np.empty((flat.size, 3), dtype=np.uint8)
        b[:, 0], b[:, 1], b[:, 2] = v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF
        payload = b.tobytes()
    elif depth == 32:
        payload = (((flat << 16) | low) & 0xFFFFFFFF).astype("<u4").tobytes()
    else:
        raise ValueError(depth)
    bps = depth // 8
    head = b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, 1, ch, rate, rate * bps * ch, bps * ch, depth) + b"data" + struct.pack("<I", len(payload))
    return head + payload


def stats_tie_cases():
    """tests/golden/stats_ties.json: streams whose `aad -c` RMSE or MSD lies on a rounding boundary of the printed six
    decimals (tie) or just outside the device's window (control); make_stats_ties_golden.py"""
    import json
    with open(os.path.join(GOLDEN, "stats_ties.json")) as f:
        return json.load(f)["cases"]


def stats_tie_input(case):
    """the int16 [frames, channels] input of a stats_ties.json case"""
    from aad_amd.synth import synth_pcm
    return synth_pcm(1, case["frames"], case["channels"], seed=case["seed"], kind=case["kind"])[0]


def build_compare_round_driver(directory):
    """tests/compare_round_driver.cpp built with g++ against aad_amd/csrc/aad_compare_round.h -> path of the executable"""
    import subprocess
    exe = os.path.join(str(directory), "compare_round_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "aad_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "compare_round_driver.cpp")], check=True)
    return exe


def compare_round(driver, rows):
    """[(n, v)] -> [(compare_reorder_bound(n), compare_crosses_boundary(v, that bound))] through the driver"""
    import subprocess
    text = "".join("%d %s\n" % (n, float(v).hex()) for n, v in rows)
    out = subprocess.run([driver], input=text, check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == 2 * len(rows)
    return [(float.fromhex(out[2 * i]), out[2 * i + 1] == "1") for i in range(len(rows))]


def reorder_bound(n):
    """delta(n), exact (fractions.Fraction): how far, relative, the RMSE or MSD of n values summed in any order lies from the
    reference's - and from the exact value.  Derived in tests/test_compare_round.py's docstring."""
    from fractions import Fraction
    u = Fraction(1, 2 ** 53)
    g = n * u / (1 - n * u)
    a = (1 + g) / (1 - g)
    d = (1 + u) / (1 - u)
    return max(a * d, (1 + a * d) / 2 * d) - 1


def exact_sum(values):
    """the exact sum (fractions.Fraction) of a float64 array: every double is an integer times a power of two; integers with the
    same exponent are summed in int64 halves that cannot overflow"""
    from fractions import Fraction
    v = np.asarray(values, dtype=np.float64).ravel()
    mant, expo = np.frexp(v)
    m = (mant * 2.0 ** 53).astype(np.int64)  # exact: |mant| < 1, 53 bits
    total = Fraction(0)
    for x in np.unique(expo):
        sel = m[expo == x]
        s = (int(np.sum(sel >> 26)) << 26) + int(np.sum(sel & ((1 << 26) - 1)))
        total += Fraction(s) * Fraction(2) ** (int(x) - 53)
    return total


def exact_squares(e):
    """e * e exactly, as three float64 arrays whose sum it is (Veltkamp's split: 26-bit halves, every product exact)"""
    e = np.asarray(e, dtype=np.float64)
    t = e * 134217729.0
    hi = t - (t - e)
    lo = e - hi
    return hi * hi, 2.0 * hi * lo, lo * lo
