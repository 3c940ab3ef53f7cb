"""Crafted int16 PCM for the ENCODERS: the corners of the recurrence that `music`, `noise` and `nyquist` (aad_amd/synth.py) never
visit - LMS weights growing until the block header needs a weight shift >= 2 (up to 13: every h*w product and the prediction sum
wrap int32), both clip rails for whole blocks, the step index pinned at 0 or travelling its whole range inside a block, the
largest |x - p| a real signal reaches.

Integer-only and bit-reproducible (numpy integer arithmetic, no libm, no floats), like aad_amd/synth.py: the GPU box rebuilds
exactly the inputs whose reference hashes are in tests/golden/crafted_pcm.json (tests/golden/make_crafted_pcm_golden.py).

A family is a function of (num_samples, channels, variant) -> int16 [num_samples, channels].  In multi-channel arrays the channels
carry different phases (or, for `mixed`, different families), so that the lanes of one wave sit in different corners at once
and, under M/S, mid and side are both non-trivial.

`cases()` is the case table (list of dicts, like bitstream_fuzz.golden_cases()): the short tier (<= 12 000 frames: every family at
every bit width under trials 0 and 2; channels 1, 2, 3, 8; M/S; block sizes 18 * ch + 24, 128, 1024, 4096; lengths that end
mid-unit and next to a block boundary) and the long tier (the period-6 tone as one chain of up to 350 436 frames).  Each case names
the corners it exists for; tests/test_crafted_pcm.py asserts that it reaches them.

TEST INFRASTRUCTURE (tests/ only).
"""
import json
import os

import numpy as np

import oracle_binding as ob
from aad_amd.synth import synth_pcm

TONE_P6 = (0, 28377, 28377, 0, -28377, -28377)  # a full-scale 8 kHz tone sampled at 48 kHz: exactly these six integers
HI, LO = 32767, -32768
_M64 = (1 << 64) - 1


def _i16(v):
    return np.ascontiguousarray(v, dtype=np.int16)


def _columns(n, channels, column):
    out = np.empty((n, channels), dtype=np.int16)
    for c in range(channels):
        out[:, c] = column(c)
    return out


def _xorshift_bits(n, seed):
    """n values in {0, 1} from a xorshift64 walk (python integers): 1 where bits 17..22 of the word are all zero, one sample in 64"""
    x = (0x9E3779B97F4A7C15 * (seed + 1)) & _M64 or 1
    out = np.empty(n, dtype=np.int16)
    for i in range(n):
        x ^= (x << 13) & _M64
        x ^= x >> 7
        x ^= (x << 17) & _M64
        out[i] = ((x >> 17) & 63) == 0
    return out


def tone_p6(n, channels=1, variant=0):
    """the literal period-6 pattern, tiled; channel c starts c + variant samples into it"""
    pat = np.array(TONE_P6, dtype=np.int16)
    return _columns(n, channels, lambda c: pat[(np.arange(n) + c + variant) % 6])


def square_p128(n, channels=1, variant=0):
    """64 samples at +32767, then 64 at -32768; channel c is 17 c + 5 variant samples ahead"""
    return _columns(n, channels, lambda c: np.where(((np.arange(n) + 17 * c + 5 * variant) // 64) % 2 == 0, HI, LO))


def dc_hi(n, channels=1, variant=0):
    """DC at the upper rail (variant 1: odd channels at the lower one)"""
    return _columns(n, channels, lambda c: LO if (variant & 1) and (c & 1) else HI)


def dc_lo(n, channels=1, variant=0):
    """DC at the lower rail (variant 1: odd channels at the upper one)"""
    return _columns(n, channels, lambda c: HI if (variant & 1) and (c & 1) else LO)


def silence(n, channels=1, variant=0):
    return np.zeros((n, channels), dtype=np.int16)


def lsb_dither(n, channels=1, variant=0):
    """Values in {0, 1} from xorshift64, a generator per (variant, channel); a 1 about once in 64 samples.  At step index 0 the step is
    1, so a lone 1 is already the largest magnitude and kicks the index up by 40 .. 256; the zeros behind it walk it back down by
    14 .. 18 a sample.  A denser dither keeps the index off 0 (every second sample: 40 % at 0); this family exists for the index
    RESTING at 0 with the kicks in between."""
    return _columns(n, channels, lambda c: _xorshift_bits(n, 16 * variant + c))


def impulses(n, channels=1, variant=0):
    """one full-scale sample every 997 (the first at 131 c + 40), zeros between; variant 1 alternates the rails"""
    def column(c):
        x = np.zeros(n, dtype=np.int16)
        at = np.arange(131 * c + 40, n, 997)
        x[at] = np.where((np.arange(len(at)) & 1) & (variant & 1), LO, HI)
        return x
    return _columns(n, channels, column)


def bursts(n, channels=1, variant=0):
    """1500 samples of zeros alternating with 1500 of a full-scale square at fs/2; channel c is 500 c + 250 variant samples ahead"""
    def column(c):
        t = np.arange(n) + 500 * c + 250 * variant
        return np.where((t // 1500) % 2 == 0, 0, np.where(t % 2 == 0, HI, LO))
    return _columns(n, channels, column)


def saw(n, channels=1, variant=0):
    """a wrapping full-scale ramp, 37 per sample; channel c starts 8191 c + 1000 variant higher"""
    return _columns(n, channels, lambda c: ((np.arange(n, dtype=np.int64) * 37 + 8191 * c + 1000 * variant) % 65536) - 32768)


def rail_stereo(n, channels=2, variant=0):
    """Even channels (L) and odd channels (R) at opposite rails: 400 samples L high / R low, 400 L low / R high, 400 of a full-scale
    square at fs/2 in antiphase, and again.  Under M/S the side (l - r) >> 1 sits at +32767, at -32768 (-65535 >> 1) and jumps
    between the two every sample; the mid is -1 throughout."""
    def column(c):
        t = np.arange(n) + 100 * variant
        seg = (t // 400) % 3
        left = np.where(seg == 0, HI, np.where(seg == 1, LO, np.where(t % 2 == 0, HI, LO)))
        return left if c % 2 == 0 else np.where(left == HI, LO, HI)
    return _columns(n, channels, column)


def mixed(n, channels=1, variant=0):
    """channel c carries family number c + variant of the list below: the lanes of one wave in different corners at once"""
    order = (tone_p6, dc_hi, silence, bursts, square_p128, dc_lo, impulses, saw, lsb_dither, rail_stereo)
    return _columns(n, channels, lambda c: order[(c + variant) % len(order)](n, 1, variant)[:, 0])


def tone_music(n, channels=2, variant=0):
    """the tone on channel 0 and `music` (aad_amd/synth.py) on the others: a diverging lane and tame ones in one wave"""
    out = synth_pcm(1, n, channels, seed=77 + variant, kind="music")[0].copy()
    out[:, 0] = tone_p6(n, 1, variant)[:, 0]
    return out


FAMILIES = {f.__name__: f for f in (tone_p6, square_p128, dc_hi, dc_lo, silence, lsb_dither, impulses, bursts, saw, rail_stereo,
                                    mixed, tone_music)}
SHORT_FAMILIES = ["tone_p6", "square_p128", "dc_hi", "dc_lo", "silence", "lsb_dither", "impulses", "bursts", "saw", "rail_stereo",
                  "mixed"]


def generate(family, num_samples, channels, variant=0):
    pcm = _i16(FAMILIES[family](num_samples, channels, variant))
    assert pcm.shape == (num_samples, channels)
    return pcm


def case_pcm(case):
    return generate(case["family"], case["num_samples"], case["channels"], case["variant"])


# ---- the corners a case can name (tests/test_crafted_pcm.py turns them into assertions) -------------------------------------------
# "shift>=N"      largest block-header weight shift of the image >= N (read from the image: any trials value)
# "shift<=N"      ... <= N (the control)
# the rest come from the instrumented restatement of the recurrence, trials 0 only:
# "sum_wraps"     at least one sample whose exact 16384 + sum h*w differs from its int32 wrap
# "clip_hi>N" / "clip_lo>N"   more than N reconstructed samples clipped at that rail
# "idx0>=90%"     the step index is 0 at 90 % of the coded samples or more
# "idx_both"      the step index reaches both 0 and 4080 (after the start)
# "dmax>N"        largest |x - p| above N

def _corners(family, bits, trials, channels):
    if trials:
        return []
    if family in ("dc_hi", "dc_lo") and bits == 2:
        return ["clip_%s>1000" % family[3:]]
    if family in ("silence", "lsb_dither", "impulses"):
        return ["idx0>=90%"]
    if family == "square_p128":
        return ["dmax>65000"]
    if family == "bursts" and bits == 4:
        return ["idx_both"]
    return []


def _short_cases():
    out = []
    k = 0
    for fi, family in enumerate(SHORT_FAMILIES):
        for bi, bits in enumerate((4, 3, 2)):
            for trials in (0, 2):
                ch = (1, 2, 3, 8)[(fi + bi + (1 if trials else 0)) % 4]
                if family == "rail_stereo":
                    ch = 2
                if family == "mixed":
                    ch = (8, 3, 2)[bi] if trials == 0 else (2, 8, 3)[bi]
                ms = bool(ch == 2 and (family == "rail_stereo" or (fi + bi) % 2 == 0))
                mbs = [18 * ch + 24, 128, 1024, 4096][(k + fi) % 4]
                if mbs < 18 * ch + 24:
                    mbs = 1024
                rc, _, spb = ob.geometry(mbs, ch, bits)
                assert rc == 0
                # lengths that end mid-unit and mid-chunk: next to a block boundary, or odd; never a multiple of 16
                n = [spb + 1, spb - 1, 11999, 3 * spb + 7, 7777, 5 * spb - 1][k % 6]
                while n > 12000:
                    n -= spb if n - spb > 5000 else 4003
                if n < 6000:  # the corners need a few thousand samples
                    n += spb * ((6000 - n) // spb + 1)
                    if n > 12000:
                        n = 11999
                if n % 16 == 0:
                    n -= 1
                variant = 1 if (ch > 1 and trials) else 0
                out.append({"name": "%s_c%d_b%d_%s_t%d_s%d_n%d" % (family, ch, bits, "ms" if ms else "lr", trials, mbs, n),
                            "tier": "short", "family": family, "variant": variant, "channels": ch, "bits": bits, "ms": ms,
                            "trials": trials, "max_block_size": mbs, "num_samples": n,
                            "corners": _corners(family, bits, trials, ch)})
                k += 1
    return out


# The long tier: prefixes of the tone that run 40 blocks past the first block whose header shift reaches 2 (trials 0: blocks 90 /
# 68 / 47 at 4 / 3 / 2 bits; trials 2: blocks 49 / 32 at 4 / 3 bits; the 2-bit search keeps the weights tame: the control).
LONG_CASES = [
    ("tone_p6", 1, 4, 0, 262080, ["shift>=2"]),
    ("tone_p6", 1, 3, 0, 289872, ["shift>=2"]),
    ("tone_p6", 1, 2, 0, 350436, ["shift>=8", "sum_wraps"]),
    ("tone_p6", 1, 4, 2, 179424, ["shift>=2"]),
    ("tone_p6", 1, 3, 2, 193248, ["shift>=2"]),
    ("tone_p6", 1, 2, 2, 350436, ["shift<=1"]),
    # stereo: 2048-byte blocks hold the 4028 samples per channel of the mono cases' 1024, so channel 0 runs the mono 2-bit chain
    ("tone_music", 2, 2, 0, 350436, ["shift>=8", "sum_wraps"]),
]


def cases():
    out = _short_cases()
    for family, ch, bits, trials, n, corners in LONG_CASES:
        mbs = 1024 * ch
        out.append({"name": "%s_c%d_b%d_lr_t%d_s%d_n%d" % (family, ch, bits, trials, mbs, n), "tier": "long", "family": family,
                    "variant": 0, "channels": ch, "bits": bits, "ms": False, "trials": trials, "max_block_size": mbs,
                    "num_samples": n, "corners": corners})
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def short_cases():
    return [c for c in cases() if c["tier"] == "short"]


def long_cases():
    return [c for c in cases() if c["tier"] == "long"]


def companions(bits, count=63):
    """`count` short mono streams (every short family, two variants, ragged lengths) to batch with a long mono case"""
    out = []
    for i in range(count):
        family = SHORT_FAMILIES[i % len(SHORT_FAMILIES)]
        n = 1 + (i * 1931 + 97 * bits) % 9000
        out.append(generate(family, n, 1, (i // len(SHORT_FAMILIES)) % 2))
    return out


def oracle_encode(case, pcm=None):
    pcm = case_pcm(case) if pcm is None else pcm
    return ob.encode(pcm, case["bits"], case["max_block_size"], 48000, case["ms"], case["trials"])


def mono_block_size(case):
    """The mono block size with the case's samples per block: without M/S a channel's recurrence does not see its neighbours, so
    channel c of an N-channel image is the mono image of column c at this block size - how the cases the
    reference cannot encode (more than two channels) are pinned to it."""
    ch, bits = case["channels"], case["bits"]
    spb = ob.geometry(case["max_block_size"], ch, bits)[2]
    size = 18 + (spb - 4) // {4: 2, 3: 8, 2: 4}[bits] * {4: 1, 3: 3, 2: 1}[bits]
    assert ob.geometry(size, 1, bits)[1:] == (size, spb)
    return size


def golden():
    """tests/golden/crafted_pcm.json as {name: record}"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crafted_pcm.json")) as f:
        return {r["name"]: r for r in json.load(f)["cases"]}


# ---- block headers of an image (failure messages, the shift corners) ---------------------------------------------------------------

def block_headers(image):
    """-> (block_size, [per block: [per channel: dict(shift, index, weights, history)]]) of an image an encoder wrote"""
    hd = ob.AadoHeader()
    buf = np.frombuffer(image, dtype=np.uint8)
    assert ob.lib().aado_get_header(buf.ctypes.data, len(buf), hd) == 0
    ch, bs = hd.num_channels, hd.block_size
    out = []
    for off in range(31, len(image), bs):
        if off + 18 * ch > len(image):
            break
        block = []
        for c in range(ch):
            f = np.frombuffer(image, dtype=">u2", count=9, offset=off + 18 * c)
            v = int(f[0])
            wh = f[1:].astype(np.int64)
            wh = np.where(wh >= 32768, wh - 65536, wh)
            block.append({"shift": v & 15, "index": v >> 4, "weights": [int(x) << (v & 15) for x in wh[0::2]],
                          "history": [int(x) for x in wh[1::2]]})
        out.append(block)
    return bs, out


def max_header_shift(image):
    return max(h["shift"] for block in block_headers(image)[1] for h in block)


def first_block_with_shift(image, at_least):
    for b, block in enumerate(block_headers(image)[1]):
        if any(h["shift"] >= at_least for h in block):
            return b
    return None


def describe_mismatch(label, got, want):
    """the assertion message of an image mismatch: first differing byte and block, and that block's header fields on both sides"""
    got, want = bytes(got), bytes(want)
    if len(got) != len(want):
        head = "%s: %d bytes, expected %d; " % (label, len(got), len(want))
    else:
        head = "%s: " % label
    n = min(len(got), len(want))
    diff = np.nonzero(np.frombuffer(got[:n], dtype=np.uint8) != np.frombuffer(want[:n], dtype=np.uint8))[0]
    at = int(diff[0]) if diff.size else n
    if at < 31:
        return head + "file header differs at byte %d: %s / %s" % (at, got[:31].hex(), want[:31].hex())
    bs, hw = block_headers(want)
    block = (at - 31) // bs
    try:
        hg = block_headers(got)[1]
    except Exception:  # a file header that does not parse
        hg = []
    return head + "first difference at byte %d = block %d + %d (block size %d)\n  got      %s\n  expected %s" % (
        at, block, (at - 31) % bs, bs, hg[block] if block < len(hg) else "-", hw[block] if block < len(hw) else "-")


def describe_pcm_mismatch(label, got, want, image=None):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s: decoded shape %s, expected %s" % (label, got.shape, want.shape)
    bad = np.argwhere(got != want)
    frame, c = (int(v) for v in bad[0])
    text = "%s: %d samples differ, the first at frame %d channel %d: %s, expected %s" % (
        label, len(bad), frame, c, got[frame:frame + 4, c].tolist(), want[frame:frame + 4, c].tolist())
    if image is not None:
        hd = ob.AadoHeader()
        buf = np.frombuffer(image, dtype=np.uint8)
        ob.lib().aado_get_header(buf.ctypes.data, len(buf), hd)
        block = frame // hd.samples_per_block
        text += "\n  block %d (+%d), header %s" % (block, frame % hd.samples_per_block, block_headers(image)[1][block])
    return text
