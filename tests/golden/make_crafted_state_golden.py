#!/usr/bin/env python3
"""Golden records of the crafted-state corpus (tests/crafted_state.py) from the COMPILED reference with a state setter and getter
(oracle/_ref/libaadref_state.so: oracle/ref_state.c standing in for the reference's encoder source).

  reached    every chain of crafted_state.REACHED_CHAINS is encoded on a fresh reference handle and the handle's records read back
             with aadref_get_lane; asserted equal to the oracle's lanes after the same chain.
  cases      per case of crafted_state.cases(): AADEncoder_SetEncodeParameter, the input records planted with aadref_set_lane (the
             step index clamped to 0 .. 4080: the reference keeps it in an int16 - the stated expectation of the `beyond` tier),
             AADEncoder_EncodeWhole of the second-call PCM, the image decoded by AADDecoder_DecodeWhole, the COMPLETE records read
             back.  Kept: the parameters, the input records, the SHA-256 of the PCM, of the image and of the decoded int16 PCM, the
             output records.  Cases of more than two channels are recorded channel by channel as mono streams at the mono block
             size with the same samples per block (crafted_pcm.mono_block_size).
  sequences  per call of crafted_state.SEQUENCES on ONE handle the same hashes and the records of the handle's lanes after the call.

Hashes, integers and parameters only: the PCM is regenerated from the generators, nothing of the reference is copied.

To regenerate, where oracle/_ref has been built (the build container):

    python tests/golden/make_crafted_state_golden.py

Output: tests/golden/crafted_state.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aad_amd  # noqa: E402
import crafted_pcm as cp  # noqa: E402
import crafted_state as cs  # noqa: E402
import oracle_binding as ob  # noqa: E402
from helpers import sha256  # noqa: E402


def decoded_sha(codec, image):
    return sha256(np.ascontiguousarray(codec.decode(image)[0], dtype="<i2").tobytes())


def reached_records(lib):
    out = {}
    for chain in cs.REACHED_CHAINS:
        case = cs.chain_case(chain)
        pcm = cs.case_pcm(case)
        enc = lib.AADEncoder_Create(case["max_block_size"], None, 0)
        try:
            image = cs.api_encode(lib, enc, case, pcm)
            got = cs.ref_get_lanes(lib, enc, case["channels"])
        finally:
            lib.AADEncoder_Destroy(enc)
        lanes = ob.fresh_lanes(case["channels"])
        assert ob.encode(pcm, case["bits"], case["max_block_size"], 48000, case["ms"], case["trials"], lanes=lanes) == image, case["name"]
        assert cs.lanes_out(lanes) == got, (case["name"], cs.lanes_out(lanes), got)
        for c, r in enumerate(got):
            out["%s/%d" % (case["name"], c)] = dict(r, chain=dict(case, pcm_sha256=sha256(pcm.tobytes()), image_sha256=sha256(image)))
    return out


def case_records(lib, codec, reached):
    records = []
    for case in cs.cases(reached):
        pcm = cs.case_pcm(case)
        recs = [cs.record(n, reached) for n in case["records"]]
        rec = dict(case)
        rec["records_in"] = recs
        rec["pcm_sha256"] = sha256(pcm.tobytes())
        rec["image_bytes"] = ob.encoded_size(case["num_samples"], case["channels"], case["bits"], case["max_block_size"])
        if case["channels"] <= 2:
            image, out = cs.ref_run(lib, case, recs, pcm)
            assert len(image) == rec["image_bytes"]
            rec["image_sha256"] = sha256(image)
            rec["decoded_sha256"] = decoded_sha(codec, image)
            rec["records_out"] = out
        else:
            rec["mono_block_size"] = cp.mono_block_size(case)
            rec["mono_image_sha256"], rec["mono_decoded_sha256"], rec["records_out"] = [], [], []
            for c in range(case["channels"]):
                column = np.ascontiguousarray(pcm[:, c:c + 1])
                image, out = cs.ref_run(lib, dict(case, ms=False), recs[c:c + 1], column, rec["mono_block_size"])
                rec["mono_image_sha256"].append(sha256(image))
                rec["mono_decoded_sha256"].append(decoded_sha(codec, image))
                rec["records_out"] += out
        records.append(rec)
    return records


def sequence_records(lib, codec):
    out = {}
    for name, calls in cs.SEQUENCES.items():
        states = []
        images = cs.api_sequence(lib, calls, lambda enc, k: states.append(cs.ref_get_lanes(lib, enc, cs.sequence_lanes(calls))))
        out[name] = []
        for call, image, state in zip(calls, images, states):
            c = cs.call_case(call)
            out[name].append(dict(c, pcm_sha256=sha256(cs.case_pcm(c).tobytes()), image_sha256=sha256(image),
                                  decoded_sha256=decoded_sha(codec, image), records_out=state))
    return out


def build():
    lib = cs.load_ref_state()
    codec = aad_amd.LegacyCodec(lib)
    reached = reached_records(lib)
    return {"generator": "tests/golden/make_crafted_state_golden.py",
            "source": "oracle/_ref/libaadref_state.so (AADEncoder_EncodeWhole, AADDecoder_DecodeWhole, aadref_set_lane, aadref_get_lane)",
            "reached": reached, "cases": case_records(lib, codec, reached), "sequences": sequence_records(lib, codec)}


def dumps(out):
    return json.dumps(out, indent=0, sort_keys=True) + "\n"


def main():
    out = build()
    with open(cs.GOLDEN, "w") as f:
        f.write(dumps(out))
    print("wrote %s: %d reached records, %d cases, %s sequence calls" % (cs.GOLDEN, len(out["reached"]), len(out["cases"]),
                                                                         [len(v) for v in out["sequences"].values()]))


if __name__ == "__main__":
    main()
