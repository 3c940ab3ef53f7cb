"""The crafted-state corpus (tests/crafted_state.py) on the CPU: the oracle pinned to the compiled reference on every case and every
field of every output record, and the corner audit that keeps the corpus honest.

1. tests/golden/crafted_state.json holds, per case, what the compiled reference with a state setter and getter
   (oracle/_ref/libaadref_state.so, oracle/ref_state.c) made of the case's input records and second-call PCM: the SHA-256 of the
   image and of its decode and the COMPLETE output records.  The oracle (ob.encode with lanes=) must reproduce all of it.  For the
   `beyond` tier the reference ran on the step index clamped to [0, 4080] - the stated expectation - and, for |w| >= 2^30, compiled
   with NDEBUG (the header's shift & 0xF wraps).
2. Corner audit: every case reaches what it names.
     first_shift==a[,b]   the first block header's weight shift per channel, read from the image (trials 0: the loaded weights')
     idx_clamp            a record's stepsize_index lies outside [0, 4080]; the first header carries the clamped index (trials 0)
     passthrough          n <= 4: no sample is coded - quantize_error out == quantize_error in, weights = the header's rounding of the
                          weights in, index unchanged, the history taps that no sample seeds are 0
     ms_both              M/S with non-zero weights on the mid and on the side lane
   and the corpus as a whole: first-block shifts 0 .. 15 all present, maxabs 32767 / 32768 / -32767 / -32768 / -32769 (both sides
   of the shift 0 / 1 boundary, both signs), every index 0, 1, 7, 8, 2040, 4079, 4080, every out-of-range index and every
   out-of-range weight record in a trials-0 case, quantize_error 0, +-1 and +-(2^31 - 1) passed through.
3. With oracle/_ref present (`ref` marker): the generator reproduces the committed file byte for byte, and both call sequences run
   live against the compiled reference on one reused handle."""
import numpy as np
import pytest

import aad_amd
import crafted_pcm as cp
import crafted_state as cs
import oracle_binding as ob
from helpers import sha256
from test_oracle_golden import extract_channel_as_mono

CASES = cs.cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def runs():
    """{name: (case, pcm, oracle image, oracle output records)}, computed once"""
    out = {}
    for c in CASES:
        pcm = cs.case_pcm(c)
        image, lanes = cs.oracle_run(c, pcm=pcm)
        out[c["name"]] = (c, pcm, image, lanes)
    return out


def test_case_table_is_the_golden_one():
    g = cs.golden()["cases"]
    assert list(g) == IDS
    keys = ("tier", "records", "family", "variant", "channels", "bits", "ms", "trials", "max_block_size", "num_samples", "corners")
    for c in CASES:
        assert {k: g[c["name"]][k] for k in keys} == {k: c[k] for k in keys}, c["name"]
        assert g[c["name"]]["records_in"] == [cs.record(n) for n in c["records"]], c["name"]
    assert 140 <= len(CASES) <= 160
    assert {c["tier"] for c in CASES} == {"reached", "synthetic", "beyond"}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_equals_golden(runs, case):
    """image, decode and every field of every output record == the compiled reference's; the PCM hash guards the generators"""
    _, pcm, image, lanes = runs[case["name"]]
    rec = cs.golden()["cases"][case["name"]]
    assert sha256(pcm.tobytes()) == rec["pcm_sha256"]
    assert len(image) == rec["image_bytes"]
    decoded = ob.decode(image)[0]
    if case["channels"] <= 2:
        assert sha256(image) == rec["image_sha256"]
        assert sha256(decoded.tobytes()) == rec["decoded_sha256"]
    else:
        for ch in range(case["channels"]):
            assert sha256(extract_channel_as_mono(image, ch, rec["mono_block_size"])) == rec["mono_image_sha256"][ch], ch
            assert sha256(np.ascontiguousarray(decoded[:, ch]).tobytes()) == rec["mono_decoded_sha256"][ch], ch
    assert lanes == rec["records_out"]


def test_reached_records_are_the_oracles_end_states():
    """the stored `reached` input records == the oracle's lanes after the chain (the generator read them from the reference handle)"""
    reached = cs.golden()["reached"]
    assert sorted(reached) == sorted(cs.REACHED_NAMES)
    for chain in cs.REACHED_CHAINS:
        case = cs.chain_case(chain)
        pcm = cs.case_pcm(case)
        lanes = ob.fresh_lanes(case["channels"])
        image = ob.encode(pcm, case["bits"], case["max_block_size"], 48000, case["ms"], case["trials"], lanes=lanes)
        for c, got in enumerate(cs.lanes_out(lanes)):
            rec = reached["%s/%d" % (case["name"], c)]
            assert sha256(pcm.tobytes()) == rec["chain"]["pcm_sha256"] and sha256(image) == rec["chain"]["image_sha256"], case["name"]
            assert got == {k: rec[k] for k in ("w", "h", "idx", "qerr")}, (case["name"], c)
    # what the chains were chosen for
    shift = {n: cs.header_shift(reached[n]["w"]) for n in reached}
    assert shift["reached_tone_p6/0"] == 13 and shift["reached_tone_music/0"] == 13 and shift["reached_tone_music/1"] <= 1, shift
    assert reached["reached_silence/0"]["w"] == [0, 0, 0, 0] and reached["reached_silence/0"]["idx"] == 0
    assert reached["reached_square_p128/0"]["idx"] >= 3900, reached["reached_square_p128/0"]["idx"]


def first_headers(image):
    return cp.block_headers(image)[1][0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_corner_audit(runs, case):
    _, pcm, image, lanes = runs[case["name"]]
    recs = [cs.record(n) for n in case["records"]]
    heads = first_headers(image)
    n = case["num_samples"]
    assert case["corners"] or case["trials"], "a trial-free case names its first header's shift"
    for corner in case["corners"]:
        if corner.startswith("first_shift=="):
            want = [int(v) for v in corner[len("first_shift=="):].split(",")]
            assert [h["shift"] for h in heads] == want, (corner, heads)
            assert want == [cs.header_shift(r["w"]) & 15 for r in recs]
        elif corner == "idx_clamp":
            outside = [c for c, r in enumerate(recs) if not 0 <= r["idx"] <= cs.IDX_MAX]
            assert outside and case["trials"] == 0
            for c in outside:
                assert heads[c]["index"] == cs.clamp_index(recs[c]["idx"]), (c, heads[c], recs[c])
        elif corner == "passthrough":
            assert n <= 4
            for c, (r, out) in enumerate(zip(recs, lanes)):
                assert out["qerr"] == r["qerr"], (c, out, r)
                x = pcm[:, c].astype(np.int64)
                if case["ms"]:
                    l, rr = pcm[:, 0].astype(np.int64), pcm[:, 1].astype(np.int64)
                    x = ((l + rr) >> 1) if c == 0 else ((l - rr) >> 1)  # both within int16
                # history[3 - k] holds sample k of the block (src/aad_encoder.c:609-615); the taps no sample seeds are 0
                assert out["h"] == [int(x[3 - t]) if 3 - t < n else 0 for t in range(4)], (c, out["h"], x.tolist())
                if case["trials"] == 0:
                    mask = ~((1 << cs.header_shift(r["w"])) - 1)
                    assert out["w"] == [w & mask for w in r["w"]] and out["idx"] == cs.clamp_index(r["idx"]), (c, out, r)
        elif corner == "ms_both":
            assert case["ms"] and all(any(r["w"]) for r in recs)
        else:
            raise AssertionError("unknown corner %r" % corner)


def test_corpus_reaches_every_corner(runs, capsys):
    """the corpus as a whole (module docstring, 2.); prints the table of first-block shifts"""
    shifts, maxabs, idx_in, beyond_t0, qerr_through, clamp = set(), set(), set(), set(), set(), set()
    lengths = {}
    for c in CASES:
        recs = [cs.record(n) for n in c["records"]]
        image = runs[c["name"]][2]
        if c["trials"] == 0:
            for h, r, name in zip(first_headers(image), recs, c["records"]):
                full = cs.header_shift(r["w"])
                if full <= 15:
                    shifts.add(h["shift"])
                maxabs.update(w for w in r["w"] if abs(w) in (32767, 32768, 32769))
                idx_in.add(r["idx"])
                if name in cs.BEYOND:
                    beyond_t0.add(name)
            if "idx_clamp" in c["corners"]:
                clamp.update(r["idx"] for r in recs if not 0 <= r["idx"] <= cs.IDX_MAX)
        if "passthrough" in c["corners"]:
            qerr_through.update(r["qerr"] for r in recs)
        spb = ob.geometry(c["max_block_size"], c["channels"], c["bits"])[2]
        n = c["num_samples"]
        kind = str(n) if n <= 5 else "4+unit" if n == 4 + cs.UNIT[c["bits"]] else {spb - 1: "spb-1", spb: "spb", spb + 1: "spb+1",
                                                                                   2 * spb + 19: "2spb+19"}[n]
        lengths[kind] = lengths.get(kind, 0) + 1
    with capsys.disabled():
        print("\nfirst-block shifts (trials 0): %s; second-call lengths: %s" % (sorted(shifts), sorted(lengths.items())))
    assert shifts == set(range(16)), sorted(shifts)
    assert {32767, 32768, -32767, -32768, -32769} <= maxabs, sorted(maxabs)
    assert {0, 1, 7, 8, 2040, 4079, 4080} <= idx_in, sorted(idx_in)
    assert clamp == {-1, 4081, 65535, cs.INT32_MIN, cs.INT32_MAX}, sorted(clamp)
    assert beyond_t0 == set(cs.BEYOND), sorted(set(cs.BEYOND) - beyond_t0)
    assert {0, 1, -1, cs.INT32_MAX, -cs.INT32_MAX} <= qerr_through, sorted(qerr_through)
    assert set(lengths) == {"1", "2", "3", "4", "5", "4+unit", "spb-1", "spb", "spb+1", "2spb+19"} and min(lengths.values()) >= 8, lengths
    formats = {(c["channels"], c["bits"], c["ms"], c["trials"], c["max_block_size"]) for c in CASES}
    for ch, ms in ((1, False), (2, False), (2, True)):
        for bits in (4, 3, 2):
            assert len({f for f in formats if f[:3] == (ch, bits, ms)}) == 2
    assert {f[3] for f in formats} == {0, 1, 2} and {3, 8} <= {f[0] for f in formats}
    assert any("ms_both" in c["corners"] and c["tier"] == t for c in CASES for t in ("synthetic",))
    # the weight records past the reference's domain: the shift the header cannot hold wraps to shift & 15
    assert sorted(cs.header_shift(cs.BEYOND[n]["w"]) for n in ("w_2p30", "w_minus_2p30_1", "w_int_max")) == [16, 16, 16]
    assert cs.header_shift(cs.BEYOND["w_int_min"]["w"]) == 1  # |INT32_MIN| wraps and never becomes the maximum: 40000 decides


def test_streams_whose_headers_cannot_hold_the_weights(runs):
    """The streams whose image does not describe the encoder's state, found by what that means: the oracle's decode of the image
    differs from the encoder's own reconstruction (crafted_state.oracle_reconstruction).  Two ways lead there - a weight magnitude
    of 2^30 or more at a block start (the header's 4-bit shift wraps; loaded with the `beyond` weight records, or grown from shift
    15 in `synthetic` cases) and INT32_MIN on a tap (the header's shift ignores it and its field reads 0) - and the corpus holds
    both, in mono, L/R and M/S, with and without trials.  Everywhere else the two are equal, which is what lets the reconstruct
    kernels write rows as they encode."""
    apart = []
    for c in CASES:
        _, pcm, image, _ = runs[c["name"]]
        if not np.array_equal(cs.oracle_reconstruction(c, pcm=pcm), ob.decode(image)[0]):
            apart.append(c)
    causes = ("w_2p30", "w_minus_2p30_1", "w_int_max", "w_int_min", "shift15_top")
    for c in apart:
        assert c["num_samples"] > 4 and any(n in causes for n in c["records"]), c["name"]
    for c in CASES:  # INT32_MIN with coded samples always parts them, whatever the other taps and the partner lane hold
        if "w_int_min" in c["records"] and c["num_samples"] > 4:
            assert c in apart, c["name"]
    alone = [c for c in apart if "w_int_min" in c["records"] and not any(n in causes[:3] for n in c["records"])]
    assert {(c["channels"], c["ms"], c["trials"] > 0) for c in alone} >= {(1, False, False), (1, False, True), (2, False, False), (2, True, True)}
    assert sum(any(n in causes[:3] or n == "shift15_top" for n in c["records"]) for c in apart) >= 5
    assert {c["tier"] for c in apart} == {"beyond", "synthetic"} and 9 <= len(apart) <= 14, [c["name"] for c in apart]


def test_sequences_oracle_equals_golden():
    """both call sequences on one carried state: per call image, decode and the handle's records == the compiled reference's"""
    for name, calls in cs.SEQUENCES.items():
        want = cs.golden()["sequences"][name]
        assert len(want) == len(calls)
        for k, ((pcm, image, lanes), rec) in enumerate(zip(cs.oracle_sequence(calls), want)):
            assert {key: rec[key] for key in cs.call_case(calls[k])} == cs.call_case(calls[k]), (name, k)
            assert sha256(pcm.tobytes()) == rec["pcm_sha256"], (name, k)
            assert sha256(image) == rec["image_sha256"], (name, k)
            assert sha256(ob.decode(image)[0].tobytes()) == rec["decoded_sha256"], (name, k)
            assert lanes == rec["records_out"], (name, k)
        assert any(not c[8] for c in calls) and any(c[7] <= 5 for c in calls)
    # what call 2 of the twelve exists for: a first block header at shift 13 on a three-sample stream
    _, image, _ = cs.oracle_sequence(cs.SEQUENCES["twelve"][:2])[1]
    assert max(h["shift"] for h in first_headers(image)) == 13


@pytest.mark.ref
def test_generator_reproduces_the_committed_file():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_crafted_state_golden",
                                                  os.path.join(os.path.dirname(cs.GOLDEN), "make_crafted_state_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(cs.GOLDEN) as f:
        assert gen.dumps(gen.build()) == f.read()


@pytest.mark.ref
def test_sequences_oracle_vs_ref_live():
    """the call sequences against the compiled reference itself, bytes and records, on one reused handle"""
    lib = cs.load_ref_state()
    codec = aad_amd.LegacyCodec(lib)
    for name, calls in cs.SEQUENCES.items():
        states = []
        images = cs.api_sequence(lib, calls, lambda enc, k: states.append(cs.ref_get_lanes(lib, enc, cs.sequence_lanes(calls))))
        for k, ((_, image, lanes), got, state) in enumerate(zip(cs.oracle_sequence(calls), images, states)):
            assert image == got, cp.describe_mismatch("sequence %s call %d" % (name, k), image, got)
            assert lanes == state, (name, k, lanes, state)
            assert np.array_equal(ob.decode(image)[0], codec.decode(got)[0]), (name, k)
