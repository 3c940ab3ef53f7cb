#!/usr/bin/env python3
"""Golden hashes of the crafted-PCM corpus (tests/crafted_pcm.py) from the COMPILED reference.

For every case of crafted_pcm.cases() the PCM is generated, encoded by oracle/_ref/libaadref.so's AADEncoder_EncodeWhole and that
image decoded by its AADDecoder_DecodeWhole; the record keeps the case's parameters and the SHA-256 of the PCM (so a generator that
drifted is noticed), of the image and of the decoded int16 PCM.  Cases of more than two channels - the reference stops at two,
src/aad.h:13 - are recorded channel by channel as the mono stream of that column at the mono block size with the same samples per
block (crafted_pcm.mono_block_size, the rule of SURVEY.md section 8c).  Hashes and parameters only: the PCM is regenerated from
the generators, nothing of the reference is copied.

To regenerate (after a change to the case table or a generator), where oracle/_ref has been built (the build container):

    python tests/golden/make_crafted_pcm_golden.py

Output: tests/golden/crafted_pcm.json.
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
import oracle_binding as ob  # noqa: E402
from helpers import sha256  # noqa: E402


def main():
    ref = aad_amd.LegacyCodec(aad_amd.load_library(ob.REF_SO, hip=False))
    records = []
    for case in cp.cases():
        pcm = cp.case_pcm(case)
        rec = dict(case)
        rec["pcm_sha256"] = sha256(pcm.tobytes())
        rec["image_bytes"] = ob.encoded_size(case["num_samples"], case["channels"], case["bits"], case["max_block_size"])
        if case["channels"] <= 2:
            image = ref.encode(pcm, case["bits"], case["max_block_size"], 48000, case["ms"], case["trials"])
            assert len(image) == rec["image_bytes"]
            decoded = ref.decode(image)[0]
            assert decoded.shape == pcm.shape
            rec["image_sha256"] = sha256(image)
            rec["decoded_sha256"] = sha256(np.ascontiguousarray(decoded, dtype="<i2").tobytes())
        else:
            rec["mono_block_size"] = cp.mono_block_size(case)
            rec["mono_image_sha256"], rec["mono_decoded_sha256"] = [], []
            for c in range(case["channels"]):
                column = np.ascontiguousarray(pcm[:, c:c + 1])
                image = ref.encode(column, case["bits"], rec["mono_block_size"], 48000, False, case["trials"])
                decoded = ref.decode(image)[0]
                rec["mono_image_sha256"].append(sha256(image))
                rec["mono_decoded_sha256"].append(sha256(np.ascontiguousarray(decoded[:, 0], dtype="<i2").tobytes()))
        records.append(rec)
    out = {"generator": "tests/golden/make_crafted_pcm_golden.py",
           "source": "oracle/_ref/libaadref.so (AADEncoder_EncodeWhole, AADDecoder_DecodeWhole)", "cases": records}
    path = os.path.join(HERE, "crafted_pcm.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (path, len(records)))


if __name__ == "__main__":
    main()
