"""GPU parity for the quad mapping's fused LMS tap update (aad_amd/csrc/aad_device.hip.h lms_first_fused: one 64-bit multiply-add
whose addend carries the weight in its upper dword), on inputs that stress the identity: carried weights at INT32_MIN, INT32_MAX
and +-2^30, block histories at both rails, and step index 4080 under alternating full-scale samples, where |qd| is at its
maximum with both signs.  tests/lms_fused_equiv.c proves the arithmetic on the CPU; this module holds every quad encoder body that
uses it to the CPU oracle.

Bar: bit-exact.  Images and COMPLETE output state records (weights, history, step index, quantize_error) == the oracle's on the
same carried records; the reconstruct caller's rows == the oracle's decode of its image.

Shapes, the smallest that reach every changed path: one block of 4 + 16 coded samples (one whole chunk), 4 + 16 + 12 (the
pipelined 12-sample tail), 4 + 5 (the short tail, encode_step), and two blocks (the state crosses a block boundary; the second
block ends in both tails).  Every length runs mono and stereo at 2, 3 and 4 bits with trials 0, 1 and 2 - kPassEncode, and the
trial search's kPassRmse / kPassBoth bodies on dual and on single trial lanes - through the interleaved int16 encoder, the planar
int16 encoder and the planar reconstruct encoder (REC 1: int16 rows), with the SIMD role off and on SIMD 0.

The records and the PCM come from tests/crafted_state.py and tests/crafted_pcm.py."""
import numpy as np
import pytest

import crafted_pcm as cp
import crafted_state as cs
import oracle_binding as ob
from aad_amd.capi import LANE_STATE_DTYPE, make_parameter

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = cs.INT32_MIN, cs.INT32_MAX
QD_MAX = {4: (32767 * 15) >> 3, 3: (32767 * 7) >> 2, 2: (32767 * 3) >> 1}  # the largest table step at the largest magnitude

# carried records: every rail of a weight on every tap, the step index at 4080 (the largest step)
RECORDS = [
    {"w": [I32_MIN, I32_MAX, 1 << 30, -(1 << 30)], "idx": 4080, "qerr": 0},
    {"w": [I32_MAX, I32_MIN, -(1 << 30), 1 << 30], "idx": 4080, "qerr": 0},
    {"w": [1 << 30, -(1 << 30), I32_MIN, I32_MAX], "idx": 4080, "qerr": 0},
    {"w": [-(1 << 30), 1 << 30, I32_MAX, I32_MIN], "idx": 4080, "qerr": 0},
    cs.record("w_int_max"),
    cs.record("alternating"),
    cs.record("shift15_top"),
    cs.record("zero"),
]


def stream_pcm(s, n, ch):
    """stream s of a launch: alternating full-scale samples from sample 0 on (the burst of `bursts`, both phases), the rails as DC
    with the channels on opposite ones, the square's edge, a ramp"""
    if s % 4 == 0:
        return np.ascontiguousarray(cp.generate("bursts", 1500 + n + (s // 4), ch, 0)[1500 + (s // 4):])
    if s % 4 == 1:
        return cp.generate("dc_hi" if s // 4 == 0 else "dc_lo", n, ch, 1)
    if s % 4 == 2:
        return np.ascontiguousarray(cp.generate("square_p128", 57 + n, ch, s // 4)[57:])
    return cp.generate("saw", n, ch, s // 4)


STREAMS = 8


def lengths(ch, bits):
    spb = ob.geometry(128, ch, bits)[2]
    assert spb >= 4 + 16 + 12
    return [(1024, 4 + 16), (1024, 4 + 16 + 12), (1024, 4 + 5), (128, spb + 4 + 16 + 12 + 5)]


_expected = {}


def expected(ch, bits, mbs, n, trials):
    """per stream (pcm, records in, oracle image, oracle records out, oracle decode), computed once per format and shared"""
    key = (ch, bits, mbs, n, trials)
    if key not in _expected:
        out = []
        for s in range(STREAMS):
            pcm = stream_pcm(s, n, ch)
            assert pcm.shape == (n, ch) and pcm.dtype == np.int16
            recs = [RECORDS[(s + 3 * c) % len(RECORDS)] for c in range(ch)]
            lanes = cs.lanes_of(recs, s)
            image = ob.encode(pcm, bits, mbs, 48000, False, trials, lanes=lanes, reset_idx=False)
            out.append((pcm, recs, image, cs.lanes_out(lanes, ch), ob.decode(image)[0]))
        _expected[key] = out
    return _expected[key]


def state_table(torch, want, ch):
    a = np.zeros(len(want) * ch, dtype=LANE_STATE_DTYPE)
    for s, (_, recs, _, _, _) in enumerate(want):
        for c, r in enumerate(recs):
            a[s * ch + c] = (r["w"], cs.garbage_history(s, c), r["idx"], r["qerr"])
    return torch.from_numpy(a.view(np.int32).reshape(-1, 10).copy()).cuda()


def check(label, want, ch, images, table, rows=None):
    got = np.ascontiguousarray(table.cpu().numpy()).view(LANE_STATE_DTYPE).reshape(-1)
    for s, (_, recs, image, records, decoded) in enumerate(want):
        assert bytes(images[s]) == image, cp.describe_mismatch("%s, stream %d" % (label, s), bytes(images[s]), image)
        for c, w in enumerate(records):
            r = got[s * ch + c]
            have = {"w": [int(v) for v in r["weight"]], "h": [int(v) for v in r["history"]], "idx": int(r["stepsize_index"]),
                    "qerr": int(r["quantize_error"])}
            assert have == w, (label, "stream %d channel %d" % (s, c), have, w, "in", recs[c])
        if rows is not None:
            assert np.array_equal(rows[s, :, :decoded.shape[0]], decoded.T), (label, "stream %d: rows differ from the decode" % s)


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_inputs_reach_the_largest_difference():
    """the streams of alternating full-scale samples at step index 4080 leave +-QD_MAX behind as quantize_error: |qd| at its
    maximum, both signs, at every bit width"""
    for bits in (2, 3, 4):
        seen = set()
        for n in (4 + 5, 4 + 16):
            for _, _, _, records, _ in expected(2, bits, 1024, n, 0):
                seen |= {r["qerr"] for r in records}
        assert {QD_MAX[bits], -QD_MAX[bits]} <= seen, (bits, sorted(seen))


@pytest.mark.parametrize("bits", [4, 3, 2])
@pytest.mark.parametrize("ch", [1, 2])
def test_quad_encoders_on_extreme_state(engine, ch, bits):
    import torch
    # (trials, trial lanes): kPassEncode alone; the search with one and with two candidates, side by side and one after the other
    searches = [(0, "dual"), (1, "dual"), (2, "dual"), (2, "single")]
    ran = 0
    try:
        for role in (None, 0):
            engine.set_simd_role(role)
            for trials, lanes in searches:
                engine.set_mapping("quad", lanes)
                for mbs, n in lengths(ch, bits):
                    param = make_parameter(ch, bits, mbs, 48000, False, trials)
                    want = expected(ch, bits, mbs, n, trials)
                    label = "%dch %d-bit trials %d (%s lanes) block %d, %d samples, SIMD role %s" % (ch, bits, trials, lanes, mbs, n, role)
                    pcm = np.stack([w[0] for w in want])
                    # interleaved int16
                    table = state_table(torch, want, ch)
                    d_img, size = engine.encode_uniform(torch.from_numpy(pcm).cuda(), param, state=table)
                    torch.cuda.synchronize()
                    assert engine.last_error() == "", (label, engine.last_error())
                    host = d_img.cpu().numpy()
                    check("encode_uniform, " + label, want, ch, [host[s, :size] for s in range(STREAMS)], table)
                    ran += 1
                    if lanes == "single" or trials == 1:
                        continue
                    x = torch.from_numpy(np.ascontiguousarray(pcm.transpose(0, 2, 1))).cuda()
                    # planar int16
                    table = state_table(torch, want, ch)
                    d_img, sizes = engine.encode_planar(x, param, state=table)
                    torch.cuda.synchronize()
                    assert engine.last_error() == "", (label, engine.last_error())
                    host = d_img.cpu().numpy()
                    check("encode_planar, " + label, want, ch, [host[s, :sizes[s]] for s in range(STREAMS)], table)
                    # planar reconstruct, int16 rows (REC 1)
                    table = state_table(torch, want, ch)
                    y, d_img, sizes = engine.reconstruct_planar(x, param, dtype=torch.int16, state=table, return_images=True)
                    torch.cuda.synchronize()
                    assert engine.last_error() == "", (label, engine.last_error())
                    host = d_img.cpu().numpy()
                    check("reconstruct_planar, " + label, want, ch, [host[s, :sizes[s]] for s in range(STREAMS)], table, y.cpu().numpy())
                    ran += 2
    finally:
        engine.set_simd_role(None)
        engine.set_mapping("auto", "dual")
    assert ran == 2 * (4 * 4 + 2 * 4 * 2)
