"""SIMD roles (AAD_HIP_OPTION_SIMD_ROLE) never change a byte: the quad encoder's four-wave workgroups with an elected worker
wave, the split decoder's elected recurrence wave over block-sized LDS rows and its scan on the waves of one SIMD pair, against
the oracle binding.

Per role (off, 0..3) and format (mono / stereo at 4, 3 and 2 bits; stereo also with mid/side): 1, 8, 9, 16 and 17 streams - a
partial quad wave (a wave holds sixteen recurrences), one workgroup against two, a ragged last workgroup - of 5 samples (a
header and one coded sample), 20 samples (less than two chunks), one full block and two blocks (the chain across a block
boundary), at max_block_size 256 and 1024.  The 1024-byte blocks of mono 3- and 2-bit streams hold more than 2048 coded samples
(2680 and 4024): the decoder's scratch fallback under a role; every other geometry keeps its residual rows in LDS, the largest
(stereo 2-bit, 1976 coded samples) close to the limit.  The device-resident uniform plans pick the quad encoder and the split
decoder for batches this small by themselves ("auto").  decode(encode(x)) under a role equals that under role off, byte for byte."""
import numpy as np
import pytest

import oracle_binding as ob
from aad_amd.capi import make_parameter
from aad_amd.synth import synth_pcm

pytestmark = pytest.mark.gpu

SIZES = (1, 8, 9, 16, 17)
FORMATS = [(ch, bits) for ch in (2, 1) for bits in (4, 3, 2)]
_want = {}


def cases(ch, bits):
    """-> [(max_block_size, mid_side, samples)]"""
    out = []
    for mbs in (256, 1024):
        spb = ob.geometry(mbs, ch, bits)[2]
        ms = ch == 2 and mbs == 256
        out += [(mbs, ms, n) for n in (5, 20, spb, 2 * spb)]
    return out


def wanted(ch, bits, mbs, ms, n):
    """the oracle's images and decoded PCM of the seventeen streams of a case, computed once -> (pcm, [image], [decoded])"""
    key = (ch, bits, mbs, ms, n)
    if key not in _want:
        pcm = synth_pcm(max(SIZES), n, ch, seed=1000 * ch + 100 * bits + mbs + n, kind="music")
        pcm[1::3] = synth_pcm(len(pcm[1::3]), n, ch, seed=77 + n, kind="noise")
        images = [ob.encode(p, bits, mbs, 48000, ms, 0) for p in pcm]
        _want[key] = (pcm, images, [ob.decode(i)[0] for i in images])
    return _want[key]


def round_trip(engine, torch, pcm, param):
    d_img, size = engine.encode_uniform(torch.from_numpy(np.ascontiguousarray(pcm)).cuda(), param)
    d_dec, _ = engine.decode_uniform(d_img, size)
    torch.cuda.synchronize()
    return d_img.cpu().numpy()[:, :size], d_dec.cpu().numpy()


def check_format(engine, role, ch, bits):
    import torch
    for mbs, ms, n in cases(ch, bits):
        pcm, want_img, want_dec = wanted(ch, bits, mbs, ms, n)
        param = make_parameter(ch, bits, mbs, 48000, ms, 0)
        for streams in SIZES:
            engine.set_simd_role(None)
            off_img, off_dec = round_trip(engine, torch, pcm[:streams], param)
            engine.set_simd_role(role)
            img, dec = round_trip(engine, torch, pcm[:streams], param)
            for s in range(streams):
                assert bytes(img[s]) == want_img[s], (role, ch, bits, mbs, n, streams, s)
                assert np.array_equal(dec[s], want_dec[s]), (role, ch, bits, mbs, n, streams, s)
            assert np.array_equal(img, off_img) and np.array_equal(dec, off_dec), (role, ch, bits, mbs, n, streams)


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("ch,bits", FORMATS)
@pytest.mark.parametrize("role", [None, 0, 1, 2, 3], ids=lambda r: "off" if r is None else "simd%d" % r)
def test_roles_keep_every_byte(engine, role, ch, bits):
    try:
        check_format(engine, role, ch, bits)
    finally:
        engine.set_simd_role(None)


def test_role_option_values(engine):
    from aad_amd import ApiError
    for bad in (4, -2, 17):
        with pytest.raises(ApiError):
            engine.set_simd_role(bad)
    engine.set_simd_role(3)
    engine.set_simd_role(None)


def test_two_pipelines_with_roles_decode_the_oracles_pcm(engine):
    """Two step pipelines alive together (four engines, four SIMDs - what bench.py times), a different batch every step: every
    step's decoded PCM is the oracle's for that step's input, and closing the pipelines leaves the engines without a role."""
    import torch
    from aad_amd.engine import Engine, EncodeDecodePipeline, _simd_roles
    others = [Engine(0, stream=torch.cuda.Stream(0)) for _ in range(3)]
    try:
        streams, samples, steps = 40, 1500, 12
        param = make_parameter(2, 4, 1024, 48000, False, 0)
        pipes = [EncodeDecodePipeline(engine, others[0], param, streams, samples, simd_roles=True),
                 EncodeDecodePipeline(others[1], others[2], param, streams, samples, simd_roles=True)]
        assert sorted(p._role_slot for p in pipes) == [0, 1]
        batches = [synth_pcm(streams, samples, 2, seed=8100 + i, kind=("music", "noise", "nyquist")[i % 3]) for i in range(3)]
        d_in = [torch.from_numpy(b).cuda() for b in batches]
        d_out = [torch.zeros_like(d_in[0]) for _ in range(steps)]
        for k in range(steps):
            pipes[k % 2].step(d_in[k % 3], d_out[k])
        torch.cuda.synchronize()
        want = [[ob.decode(ob.encode(b[s], 4, 1024))[0] for s in range(0, streams, 3)] for b in batches]
        for k in range(steps):
            got = d_out[k].cpu().numpy()
            for i, s in enumerate(range(0, streams, 3)):
                assert np.array_equal(got[s], want[k % 3][i]), (k, s)
        for p in pipes:
            p.close()
        assert _simd_roles[0].taken == [False, False]
    finally:
        for e in others:
            e.close()
