"""Crafted CARRIED PREDICTOR STATE for the encoders: the third thing a caller controls besides images (tests/bitstream_fuzz.py) and
PCM (tests/crafted_pcm.py).  A state record (struct AADHipLaneState; the reference's struct AADEncodeProcessor of a reused handle)
holds weight[4], history[4], stepsize_index and quantize_error per channel; music and noise leave tame ones behind.  Here a second
call starts from records that put the FIRST block header at a weight shift of 2 .. 15 (PCM alone reaches 13), on both sides of the
shift 0 / 1 boundary, with the step index at its ends, with quantize_error at its ends, with different records on the channels of
one stream - and is 1 .. 5 samples short, or ends next to a block boundary.

Integer-only and reproducible like tests/crafted_pcm.py, whose families make the second call's PCM.  A case has an input record per
channel (by name: record()), a second-call PCM (family, variant, num_samples), parameters and the corners it exists for;
tests/test_crafted_state.py asserts that it reaches them.  Tiers:

  reached    end states of crafted-PCM chains (REACHED_CHAINS), computed once by tests/golden/make_crafted_state_golden.py from the
             compiled reference and stored in tests/golden/crafted_state.json
  synthetic  inside the reference's domain: |w| <= 2^30 - 1, index 0 .. 4080
  beyond     no reference contract.  stepsize_index outside [0, 4080]: the expected result is the oracle's on the index clamped to
             [0, 4080] (what the kernels do on load, include/aad_hip.h).  |w| >= 2^30 and INT32_MIN: the header's shift & 0xF
             wraps; the expected result is the reference compiled with NDEBUG (its assertion on the shift compiled out).
  sequence   call sequences on ONE reused handle that change bits, M/S, block size and channel count between calls, some calls
             without AADEncoder_SetEncodeParameter in front (the step index carried)

The history of an input record is garbage on purpose (garbage_history): every block start overwrites it.

TEST INFRASTRUCTURE (tests/ only).
"""
import ctypes as C
import json
import os

import numpy as np

import crafted_pcm as cp
import oracle_binding as ob

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
IDX_MAX = 4080
UNIT = {4: 2, 3: 8, 2: 4}  # samples of a channel in one pack unit
SECOND_CALL_FAMILIES = ["tone_p6", "square_p128", "dc_hi", "silence", "saw", "rail_stereo"]
REF_STATE_SO = os.path.join(ob.ROOT, "oracle", "_ref", "libaadref_state.so")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crafted_state.json")


def header_shift(w):
    """the block header's weight shift of four weights as the reference computes it (src/aad_encoder.c:623-636; compiled with NDEBUG
    the absolute value of INT32_MIN wraps to itself and never becomes the maximum); the header field keeps shift & 15"""
    maxabs = 0
    for v in w:
        a = v if v > 0 else -v
        if a > INT32_MAX:
            a = INT32_MIN
        maxabs = max(maxabs, a)
    shift = 0
    while maxabs > 32767:
        maxabs >>= 1
        shift += 1
    return shift


def clamp_index(idx):
    return min(max(idx, 0), IDX_MAX)


def garbage_history(i, c):
    """what an input record's history holds: four values no PCM can leave there (past int16), different per stream and channel"""
    return [0x12345678 - 977 * i - c, -0x0BADF00D + i, 0x7FFFFFFF - c, INT32_MIN + 31 * i + c]


# ---- records ------------------------------------------------------------------------------------------------------------------------

_IDX = (0, 1, 7, 8, 2040, 4079, 4080)
_QERR = (0, 1, -1, INT32_MAX, -INT32_MAX)


def _rec(w, idx=0, qerr=0):
    return {"w": [int(v) for v in w], "idx": int(idx), "qerr": int(qerr)}


def _synthetic():
    out = {}
    for k in range(1, 16):  # the largest magnitude just above 2^(14 + k): shift k exactly
        top = (1 << (14 + k)) + 12345
        out["shift%d" % k] = _rec([top, -(1 << (13 + k)) - 5, (1 << k) | 1, -(top - 1)], _IDX[k % 7], _QERR[k % 5])
    out["shift15_top"] = _rec([(1 << 30) - 1, -((1 << 30) - 1), 12345, -1], 4080, INT32_MAX)
    out["shift14_top"] = _rec([(1 << 29) - 1, -((1 << 29) - 1), 1 << 28, -77777], 2040, -INT32_MAX)
    out["max32767"] = _rec([32767, -5, 100, 0], 8, 1)
    out["max32768"] = _rec([3, 32768, 1, -1], 7, -1)
    out["min32767"] = _rec([-32767, 7, 3, -9], 4079, 0)
    out["min32768"] = _rec([7, 3, -32768, -9], 1, INT32_MAX)
    out["min32769"] = _rec([0, -1, 2, -32769], 2040, -INT32_MAX)
    out["huge_tap"] = _rec([0, 0, (1 << 30) - 1, 0], 0, 1)
    out["alternating"] = _rec([(1 << 28) + 1, -(1 << 28) - 1, (1 << 28) + 1, -(1 << 28) - 1], 4080, -1)
    out["zero"] = _rec([0, 0, 0, 0], 0, 0)
    for v in _IDX:
        out["idx%d" % v] = _rec([1200, -800, 300, -40], v, _QERR[v % 5])
    return out


def _beyond():
    out = {}
    for name, v in (("idx_minus1", -1), ("idx4081", 4081), ("idx65535", 65535), ("idx_int_min", INT32_MIN), ("idx_int_max", INT32_MAX)):
        out[name] = _rec([(1 << 17) + 12345, -40000, 300, -(1 << 16)], v, _QERR[len(out) % 5])
    out["w_2p30"] = _rec([1 << 30, 5, -7, 9], 8, 1)
    out["w_minus_2p30_1"] = _rec([77, -(1 << 30) - 1, 1 << 29, -3], 2040, -1)
    out["w_int_min"] = _rec([INT32_MIN, 40000, -3, 2], 7, INT32_MAX)
    out["w_int_max"] = _rec([INT32_MAX, -INT32_MAX, 1, -1], 4080, -INT32_MAX)
    return out


SYNTHETIC = _synthetic()
BEYOND = _beyond()

# (name, family, variant, channels, bits, ms, trials, max_block_size, num_samples): the state the chain leaves is the record(s)
REACHED_CHAINS = [
    ("tone_music", "tone_music", 0, 2, 2, False, 0, 2048, 350436),   # lane 0 diverged (shift 13), lane 1 tame
    ("dc_hi", "dc_hi", 1, 2, 2, False, 0, 1024, 6001),               # lane 0 at the upper rail, lane 1 at the lower
    ("bursts", "bursts", 0, 2, 3, False, 2, 1024, 7777),
    ("tone_p6", "tone_p6", 0, 1, 2, False, 0, 1024, 350436),          # shift 13
    ("silence", "silence", 0, 1, 4, False, 0, 1024, 4000),           # all zero, index 0
    ("square_p128", "square_p128", 0, 1, 4, False, 0, 1024, 6085),  # index 4037: near 4080
    ("dc_lo", "dc_lo", 0, 1, 4, False, 0, 128, 5003),
]
REACHED_NAMES = ["reached_%s/%d" % (c[0], k) for c in REACHED_CHAINS for k in range(c[3])]


def chain_case(chain):
    name, family, variant, ch, bits, ms, trials, mbs, n = chain
    return {"name": "reached_" + name, "family": family, "variant": variant, "channels": ch, "bits": bits, "ms": ms, "trials": trials,
            "max_block_size": mbs, "num_samples": n}


_golden = None


def golden():
    """tests/golden/crafted_state.json: {"reached": {name: record}, "cases": {name: record}, "sequences": {name: [call records]}}"""
    global _golden
    if _golden is None:
        with open(GOLDEN) as f:
            g = json.load(f)
        _golden = {"reached": g["reached"], "cases": {r["name"]: r for r in g["cases"]}, "sequences": g["sequences"]}
    return _golden


def record(name, reached=None):
    """a record by name -> {"w", "idx", "qerr"}; the `reached` ones come from the golden file unless the generator passes them"""
    if name in SYNTHETIC:
        return SYNTHETIC[name]
    if name in BEYOND:
        return BEYOND[name]
    r = (golden()["reached"] if reached is None else reached)[name]
    return {"w": r["w"], "idx": r["idx"], "qerr": r["qerr"]}


def tier_of(names):
    if any(n in BEYOND for n in names):
        return "beyond"
    return "reached" if any(n.startswith("reached_") for n in names) else "synthetic"


# ---- the case table -----------------------------------------------------------------------------------------------------------------

def _mbs(kind, ch):
    return (18 * ch + 24, 128, 1024)[kind]


def formats():
    """eighteen (channels, bits, ms, trials, max_block_size): mono, L/R and M/S at 4, 3 and 2 bits, twice each, so that every
    trials value and block size meets every bit width and channel mode"""
    out = []
    for ci, (ch, ms) in enumerate(((1, False), (2, False), (2, True))):
        for bi, bits in enumerate((4, 3, 2)):
            for j in range(2):
                out.append((ch, bits, ms, (ci + bi + 2 * j) % 3, _mbs((ci + 2 * bi + j) % 3, ch)))
    return out


def lengths(ch, bits, mbs):
    spb = ob.geometry(mbs, ch, bits)[2]
    return [1, 2, 3, 4, 5, 4 + UNIT[bits], spb - 1, spb, spb + 1, 2 * spb + 19]


def _case(names, family, variant, ch, bits, ms, trials, mbs, n, reached):
    recs = [record(r, reached) for r in names]
    corners = []
    if trials == 0:  # the first header is the loaded weights' (the trial search moves them before it)
        corners.append("first_shift==" + ",".join(str(header_shift(r["w"]) & 15) for r in recs))
        if any(r["idx"] != clamp_index(r["idx"]) for r in recs):
            corners.append("idx_clamp")
    if n <= 4:
        corners.append("passthrough")
    if ms and all(any(r["w"]) for r in recs):
        corners.append("ms_both")
    return {"name": "%s_%s%d_c%d_b%d_%s_t%d_s%d_n%d" % ("+".join(names), family, variant, ch, bits, "ms" if ms else "lr", trials, mbs, n),
            "tier": tier_of(names), "records": list(names), "family": family, "variant": variant, "channels": ch, "bits": bits,
            "ms": ms, "trials": trials, "max_block_size": mbs, "num_samples": n, "corners": corners}


def cases(reached=None):
    """Eight second-call cases per format - five on synthetic records, two on reached ones, one beyond - over four of the ten
    lengths, two cases at each (encode_uniform's equal-length subsets); the lengths, families and records rotate over the formats
    so that every record meets several formats and lengths.  Then a 3- and an 8-channel case with a different record on every
    channel."""
    pool = {"synthetic": list(SYNTHETIC), "reached": REACHED_NAMES, "beyond": list(BEYOND)}
    pairs = [i for i in range(len(REACHED_NAMES) - 1) if REACHED_NAMES[i].endswith("/0") and REACHED_NAMES[i + 1].endswith("/1")]
    pairs += [i for i in range(len(REACHED_NAMES) - 1) if REACHED_NAMES[i].endswith("/0") and REACHED_NAMES[i + 1].endswith("/0")]
    at = {}  # the trial-free formats walk the pools on their own: there the first header is the loaded record's, every record gets one
    out = []
    k = 0
    for f, (ch, bits, ms, trials, mbs) in enumerate(formats()):
        lens = lengths(ch, bits, mbs)
        for slot in range(8):
            tier = ("synthetic", "reached", "synthetic", "beyond", "synthetic", "reached", "synthetic", "synthetic")[slot]
            if tier == "reached" and ch == 2:  # both lanes of a stereo chain (one diverged, one tame), or two mono chains' lanes
                first = pairs[at.get("pair", 0) % len(pairs)]
                names = REACHED_NAMES[first:first + 2]
                at["pair"] = at.get("pair", 0) + 1
            else:
                key = (tier, trials == 0)
                names = [pool[tier][(at.get(key, 0) + c) % len(pool[tier])] for c in range(ch)]
                at[key] = at.get(key, 0) + ch
            n = lens[(4 * f + slot // 2) % 10]
            family = SECOND_CALL_FAMILIES[k % 6]
            out.append(_case(names, family, (k // 6) % 2, ch, bits, ms, trials, mbs, n, reached))
            k += 1
    spb3, spb8 = ob.geometry(128, 3, 4)[2], ob.geometry(1024, 8, 2)[2]
    out.append(_case(["shift15_top", "min32768", "shift9"], "saw", 1, 3, 4, False, 0, 128, 2 * spb3 + 19, reached))
    out.append(_case(["shift14_top", "idx4079", "alternating", "zero", "max32768", "shift2", "huge_tap", "shift12"], "tone_p6", 0, 8, 2,
                     False, 2, 1024, spb8 + 1, reached))
    # INT32_MIN on a tap next to tame ones: the header's shift stays small and the tap's 16-bit field reads 0 - a decoder runs the
    # block without that weight.  More than four samples, mono and L/R, in formats of the table above, with and without trials.
    fm = formats()
    for names, ch, ms, trials, family, length in ((["w_int_min"], 1, False, 0, "dc_hi", 9), (["w_int_min"], 1, False, 2, "saw", 6),
                                                  (["shift3", "w_int_min"], 2, False, 0, "tone_p6", 9),
                                                  (["w_int_min", "idx2040"], 2, True, 1, "rail_stereo", 8)):
        _, bits, _, _, mbs = [f for f in fm if f[0] == ch and f[2] == ms and (f[3] == 0) == (trials == 0) and f[3] == trials][0]
        out.append(_case(names, family, 0, ch, bits, ms, trials, mbs, lengths(ch, bits, mbs)[length], reached))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def case_pcm(case):
    return cp.generate(case["family"], case["num_samples"], case["channels"], case["variant"])


# The call sequences: (family, variant, channels, bits, ms, trials, max_block_size, num_samples, set_parameter).  set_parameter
# False: the call follows the one before with no AADEncoder_SetEncodeParameter in between - same parameters, the step index carried.
SEQUENCES = {
    "twelve": [
        ("tone_music", 0, 2, 2, False, 0, 2048, 350436, True),
        ("dc_hi", 0, 2, 4, True, 0, 1024, 3, True),          # first block header at shift 13
        ("tone_p6", 0, 2, 3, False, 2, 128, 2, True),
        ("square_p128", 0, 2, 4, True, 2, 1024, 5000, True),
        ("tone_p6", 0, 1, 2, False, 0, 1024, 40000, True),
        ("silence", 0, 1, 4, False, 2, 60, 1, True),
        ("rail_stereo", 0, 2, 2, True, 1, 4096, 4097, True),
        ("saw", 0, 2, 4, False, 0, 1024, 900, True),
        ("saw", 1, 2, 4, False, 0, 1024, 3, False),
        ("bursts", 0, 2, 4, False, 0, 1024, 2500, False),
        ("dc_lo", 1, 2, 4, False, 0, 1024, 4, False),
        ("impulses", 1, 2, 3, True, 0, 256, 7777, True),
    ],
    "mono": [
        ("square_p128", 0, 1, 4, False, 0, 128, 3000, True),
        ("silence", 0, 1, 3, False, 2, 42, 1, True),
        ("saw", 0, 1, 3, False, 2, 42, 2, False),
        ("dc_hi", 0, 1, 3, False, 2, 42, 5, False),
        ("tone_p6", 0, 1, 2, False, 1, 1024, 20000, True),
        ("dc_hi", 0, 1, 4, False, 0, 1024, 4, True),
        ("saw", 1, 1, 4, False, 0, 1024, 3, False),
        ("bursts", 0, 1, 4, False, 0, 1024, 2500, False),
        ("rail_stereo", 1, 1, 3, False, 2, 60, 777, True),
    ],
}
SEQUENCE_MAX_BLOCK_SIZE = 4096  # what the reused handle is created with


def call_case(call):
    family, variant, ch, bits, ms, trials, mbs, n, set_parameter = call
    return {"family": family, "variant": variant, "channels": ch, "bits": bits, "ms": ms, "trials": trials, "max_block_size": mbs,
            "num_samples": n, "set_parameter": set_parameter}


# ---- the oracle on a case -----------------------------------------------------------------------------------------------------------

def lanes_of(records, first_stream=0):
    """AadoLane array from input records: the index clamped (the stated expectation of the `beyond` tier), garbage history"""
    lanes = ob.fresh_lanes(len(records))
    for c, r in enumerate(records):
        lanes[c].w[:] = r["w"]
        lanes[c].h[:] = garbage_history(first_stream, c)
        lanes[c].idx = clamp_index(r["idx"])
        lanes[c].qerr = r["qerr"]
    return lanes


def lanes_out(lanes, count=None):
    return [{"w": list(l.w), "h": list(l.h), "idx": int(l.idx), "qerr": int(l.qerr)} for l in list(lanes)[:count]]


def oracle_run(case, reached=None, pcm=None):
    """-> (image, output records) of the oracle for a case: the second call on the case's records"""
    pcm = case_pcm(case) if pcm is None else pcm
    lanes = lanes_of([record(n, reached) for n in case["records"]])
    image = ob.encode(pcm, case["bits"], case["max_block_size"], 48000, case["ms"], case["trials"], lanes=lanes, reset_idx=False)
    return image, lanes_out(lanes)


def sequence_lanes(calls):
    """The lanes of a sequence's handle that its records keep: those of the first call, which no later call exceeds.  (A lane that no
    call has coded a sample on is not comparable: the reference's AADEncoder_Create leaves its quantize_error uninitialised.)"""
    assert max(c[2] for c in calls) == calls[0][2] and calls[0][7] > 4
    return calls[0][2]


def oracle_reconstruction(case, reached=None, pcm=None):
    """The ENCODER's own reconstruction of the case's second call, int16 [n, C] (L/R).  It is the decode of the image wherever every
    block header can carry the encoder's weights.  A weight magnitude of 2^30 or more at a block start (loaded, or grown there)
    wraps the header's 4-bit shift, and INT32_MIN - which the header's shift ignores - reads back as 0: a decoder then runs that
    block on other weights, and the decode of the image parts from what the encoder holds."""
    pcm = case_pcm(case) if pcm is None else pcm
    lanes = lanes_of([record(n, reached) for n in case["records"]])
    recon = np.zeros(pcm.shape, dtype=np.int16)
    ob.encode(pcm, case["bits"], case["max_block_size"], 48000, case["ms"], case["trials"], lanes=lanes, reset_idx=False, recon=recon)
    return recon


def oracle_sequence(calls):
    """-> per call (pcm, image, records of the handle's lanes after the call) of the oracle on one carried state"""
    lanes = ob.fresh_lanes(sequence_lanes(calls))
    out = []
    for call in calls:
        c = call_case(call)
        pcm = case_pcm(c)
        image = ob.encode(pcm, c["bits"], c["max_block_size"], 48000, c["ms"], c["trials"], lanes=lanes, reset_idx=c["set_parameter"])
        out.append((pcm, image, lanes_out(lanes)))
    return out


# ---- a library with the reference's encoder API (the compiled reference, or this project's legacy handle) ----------------------------

def api_encode(lib, encoder, case, pcm, set_parameter=True, after_set=None):
    """AADEncoder_SetEncodeParameter (unless set_parameter is False), after_set(encoder) - where the generator plants its records -
    and AADEncoder_EncodeWhole on a handle -> bytes"""
    from aad_amd.capi import ApiError, _planar_pointers, make_parameter
    n, ch = pcm.shape
    planar = np.ascontiguousarray(pcm.T.astype(np.int32))
    if set_parameter:
        param = make_parameter(ch, case["bits"], case["max_block_size"], 48000, case["ms"], case["trials"])
        rc = lib.AADEncoder_SetEncodeParameter(encoder, C.byref(param))
        if rc != 0:
            raise ApiError("AADEncoder_SetEncodeParameter", rc)
    if after_set is not None:
        after_set(encoder)
    cap = ob.encoded_size(n, ch, case["bits"], case["max_block_size"]) + 64
    out = np.zeros(cap, dtype=np.uint8)
    size = C.c_uint32(0)
    rc = lib.AADEncoder_EncodeWhole(encoder, _planar_pointers(planar), n, out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(size))
    if rc != 0:
        raise ApiError("AADEncoder_EncodeWhole", rc)
    return out[:size.value].tobytes()


def api_sequence(lib, calls, after_call=None):
    """the calls on one handle -> [image]; after_call(encoder, k): where the generator reads the handle's state"""
    from aad_amd.capi import ApiError
    enc = lib.AADEncoder_Create(SEQUENCE_MAX_BLOCK_SIZE, None, 0)
    if not enc:
        raise ApiError("AADEncoder_Create", 1)
    images = []
    try:
        for k, call in enumerate(calls):
            c = call_case(call)
            images.append(api_encode(lib, enc, c, case_pcm(c), c["set_parameter"]))
            if after_call is not None:
                after_call(enc, k)
    finally:
        lib.AADEncoder_Destroy(enc)
    return images


def load_ref_state():
    """oracle/_ref/libaadref_state.so: the reference's API plus aadref_set_lane / aadref_get_lane (oracle/ref_state.c)"""
    import aad_amd
    lib = aad_amd.load_library(REF_STATE_SO, hip=False)
    i32p = C.POINTER(C.c_int32)
    lib.aadref_set_lane.argtypes = [C.c_void_p, C.c_uint32, i32p, C.c_int32, C.c_int32]
    lib.aadref_set_lane.restype = C.c_int
    lib.aadref_get_lane.argtypes = [C.c_void_p, C.c_uint32, i32p, i32p, i32p, i32p]
    lib.aadref_get_lane.restype = C.c_int
    return lib


def ref_get_lanes(lib, encoder, count):
    out = []
    for c in range(count):
        w, h, idx, qerr = (C.c_int32 * 4)(), (C.c_int32 * 4)(), C.c_int32(0), C.c_int32(0)
        assert lib.aadref_get_lane(encoder, c, w, h, C.byref(idx), C.byref(qerr)) == 0
        out.append({"w": list(w), "h": list(h), "idx": idx.value, "qerr": qerr.value})
    return out


def ref_set_lanes(lib, encoder, records):
    for c, r in enumerate(records):
        assert lib.aadref_set_lane(encoder, c, (C.c_int32 * 4)(*r["w"]), clamp_index(r["idx"]), r["qerr"]) == 0


def ref_run(lib, case, records, pcm, max_block_size=None):
    """the compiled reference's second call on `records` -> (image, output records)"""
    from aad_amd.capi import ApiError
    mbs = case["max_block_size"] if max_block_size is None else max_block_size
    enc = lib.AADEncoder_Create(mbs, None, 0)
    if not enc:
        raise ApiError("AADEncoder_Create", 1)
    try:
        image = api_encode(lib, enc, dict(case, max_block_size=mbs), pcm, True, lambda e: ref_set_lanes(lib, e, records))
        return image, ref_get_lanes(lib, enc, pcm.shape[1])
    finally:
        lib.AADEncoder_Destroy(enc)
