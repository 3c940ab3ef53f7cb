"""Every compiled encoder and decoder kernel, launched once: each record of tests/encode_matrix.py's case table that names a case of
this file is run by that case - the encoders grouped by (IN, REC, SEG, BITS), the decoders by kernel family and BITS - and the
closing case holds the number of records run per kernel to the table's.

Bar: bit-exact, no tolerance anywhere.  Images == the oracle's (tests/oracle_binding.encode; segmented plans: tests/segment_oracle.
segmented_encode at (L, W) = (2, 1)); reconstructed rows == the oracle's decode of that image (float32 rows as bit patterns),
untouched behind a stream's end and everywhere else in their buffer; statistics == the exact integer sums of q(x) - decoded; a
decoder's PCM == the oracle's decode.  Every output buffer is pre-filled with a pattern that must survive around what a run owns.
The expected data depends on (bits, channels, M/S, trials, segmentation, quantised input) alone, never on the kernel kind: it is
computed once per such key (expected) and shared by the records.

Which kernel ran.  Before a launch the plan of exactly this batch on this device is asked from aad_launch_policy.h
(tests/launch_policy_driver.cpp; the split decoder under a SIMD role: tests/simd_role_policy_driver.cpp, the same rows with that
knob) and must name the record's kernel kind; the step from the plan and the arguments to the template arguments is the switch
that tests/encode_matrix.py transcribes.  A case whose plan names another kernel fails.

Witnesses, asserted on the CPU before the device is asked, so that a NEIGHBOURING instantiation could not pass: the M/S image
differs from the L/R image of the same samples (whose channels differ); the trials = 2 image differs from the trials = 0 image in
at least one block; the segmented image differs from the serial one for at least one stream; the float32 rows hold samples whose
quantisation differs from truncation and from a clamp applied after the conversion; the decoded rows differ from the input, so the
statistics are not trivially zero, and in every channel some row's largest error is its last sample's alone (those streams end
on a jump to the rail), so a maximum that misses the end of a unit tail is another number.  QUAD, DUAL, RING and the streamed stores (NT) change no byte by definition, and neither do
LDSRES and ROLE of the split decoder: for those the policy assertion is the evidence.

Shapes: the smallest at which these kernels can still go wrong.  max_block_size 256 and 301 in alternate cases (other unit
tails), 40 streams (more than a wave of quad recurrences, a last wave that is not full in either mapping), lengths cycling through
1, 3, 4, 17, spb - 5, spb, spb + 1, 2 spb + 13, 7 spb + 9; CHF = 0 with three channels; planar rows at a channel stride above T
with garbage between and behind them; float32 input as tests/test_gpu_planar_encode.py builds it (ties, values past full scale,
NaNs, infinities).  The decoders that need another geometry take the smallest one their plan accepts (_decoder_geometry)."""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

import encode_matrix as em
import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import LANE_MAPPINGS, SIMD_ROLE_OFF, STREAM_DESC_DTYPE, TRIAL_LANES, make_parameter
from aad_amd.engine import parse_header
from aad_amd.synth import synth_pcm
from test_gpu_planar_encode import image_table, lay_out, make_rows, q

pytestmark = pytest.mark.gpu

STREAMS = 40
SEGMENTATION = (2, 1)         # (L, W): several chains per stream from 2 spb + 13 frames on
IMG_CANARY = 0xA5             # tests/test_gpu_planar_encode.CANARY, what image_table's gaps are held to
PCM_CANARY = 0x5A5A
ROW_CANARY_I16 = 0x5A5A
ROW_CANARY_F32 = 0x7FC5A5A5   # a NaN: float32 rows are compared as bit patterns
STATS_CANARY = -0x0123456789ABCDEF
LDS_PER_CU = 163840           # gfx950
ENV_KNOBS = ("AAD_HIP_ENCODE_RING", "AAD_HIP_DECODE_NT_MIN", "AAD_HIP_MAPPING", "AAD_HIP_ENCODE_LDS_PAD", "AAD_HIP_DECODE_LDS_PAD")

JUMP_AT_END = (3, 4, 7)       # of the nine lengths: the streams of 17, spb - 5 and 2 spb + 13 frames end on a jump to the rail
RAN = collections.Counter()   # (kernel, args) -> launches compared


def block_lengths(spb):
    return [1, 3, 4, 17, spb - 5, spb, spb + 1, 2 * spb + 13, 7 * spb + 9]


def stream_lengths(spb, streams=STREAMS):
    cycle = block_lengths(spb)
    return [cycle[i % len(cycle)] for i in range(streams)]


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    """two contexts: "plain" with no measurement aid in its environment, "ring" created under AAD_HIP_ENCODE_RING=2 (every
    geometry that can take the byte ring; a context reads it when it is created)"""
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    made = {}
    with pytest.MonkeyPatch.context() as mp:
        for name in ENV_KNOBS:
            mp.delenv(name, raising=False)
        made["plain"] = Engine(0)
        mp.setenv("AAD_HIP_ENCODE_RING", "2")
        made["ring"] = Engine(0)
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    """asks aad_launch_policy.h, the header the launches are planned with, for the plan of a batch on this device"""
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    out = tmp_path_factory.mktemp("encode_matrix_policy")
    exes = {}
    for name in ("launch_policy_driver", "simd_role_policy_driver"):
        exes[name] = str(out / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(os.path.dirname(here), "aad_amd", "csrc"), "-o",
                        exes[name], os.path.join(here, name + ".cpp")], check=True)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    memo = {}

    def ask(exe, line):
        if (exe, line) not in memo:
            memo[(exe, line)] = subprocess.run([exes[exe]], input=line + "\n", check=True, capture_output=True, text=True).stdout.split()
        return memo[(exe, line)]

    class Policy:
        @staticmethod
        def encode(rec, mapping, lanes, ring_knob, bits, ch, streams, trials, block_size, ring_ok):
            """-> (kernel kind, the TRIALS instantiation)"""
            f = ask("launch_policy_driver", "%s %d %d %d %d %d -1 -1 0 %d %d %d %d %d %d" % (
                "R" if rec else "E", cus, LDS_PER_CU, LANE_MAPPINGS[mapping], TRIAL_LANES[lanes], ring_knob, bits, ch, streams, trials,
                block_size, ring_ok))
            return f[0], int(f[1])

        @staticmethod
        def decode(mapping, simd_role, batch):
            """-> (kernel kind, streamed stores, under a role)"""
            f = ask("simd_role_policy_driver", "D %d %d %d 0 1 -1 -1 0 %d %s" % (cus, LDS_PER_CU, LANE_MAPPINGS[mapping], simd_role,
                                                                                " ".join(str(int(v)) for v in batch)))
            return f[0], int(f[1]), int(f[7]) != 0
    return Policy


# ---- what a case encodes and what the oracle makes of it, on the CPU ----------------------------------------------------------------
Samples = collections.namedtuple("Samples", "lengths rows pcm spb block_size")  # rows: [C, n] of the input type; pcm: q(rows).T
Expected = collections.namedtuple("Expected", "images decoded stats")


@functools.lru_cache(maxsize=None)
def samples(ch, bits, mbs, f32):
    """the input of every record with these channels, bits and block size: int16 rows, or float32 rows with ties, values past full
    scale and the special bit patterns"""
    rc, block_size, spb = ob.geometry(mbs, ch, bits)
    assert rc == 0 and spb > 5 + 17
    lengths = stream_lengths(spb)
    rng = np.random.default_rng(1000 * ch + 10 * bits + mbs)
    rows = make_rows(rng, ch, lengths, np.float32 if f32 else np.int16, seed=17 * ch + bits + mbs)
    for i, r in enumerate(rows):  # a jump to the rail on the last frame of some streams: the largest error of the row is its last sample's
        if i % len(block_lengths(spb)) in JUMP_AT_END:
            for c in range(ch):
                r[c, -1] = (-32768 if q(r[c, -2:-1])[0] >= 0 else 32767) / (32768.0 if f32 else 1)  # away from the sample before
    pcm = [np.ascontiguousarray(q(r).T) for r in rows]
    if ch == 2:
        assert any(not np.array_equal(p[:, 0], p[:, 1]) for p in pcm)  # M/S has something to do
    if f32:
        with np.errstate(invalid="ignore"):  # the signalling NaNs among the special bit patterns
            x = np.concatenate([r.reshape(-1) for r in rows]).astype(np.float64)
        got = np.concatenate([p.T.reshape(-1) for p in pcm]).astype(np.int64)
        fin = np.isfinite(x)
        scaled = x[fin] * 32768.0
        truncated = np.clip(np.trunc(scaled), -32768, 32767).astype(np.int64)
        assert (got[fin] != truncated).sum() > 100, "no sample whose rounding differs from truncation"
        inside = np.abs(scaled) < 2.0 ** 62
        wrapped = np.round(scaled[inside]).astype(np.int64).astype(np.int16).astype(np.int64)  # converted first: nothing left to clamp
        assert (got[fin][inside] != wrapped).sum() > 10, "no sample past full scale"
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    return Samples(lengths, rows, pcm, spb, block_size)


@functools.lru_cache(maxsize=None)
def expected(ch, bits, ms, trials, seg, mbs, f32):
    """images, decodes and exact statistics of the samples, from the oracle alone"""
    s = samples(ch, bits, mbs, f32)
    if seg:
        images = [so.segmented_encode(p, bits, SEGMENTATION[0], SEGMENTATION[1], max_block_size=mbs, ms=bool(ms), trials=trials) for p in s.pcm]
    else:
        images = [ob.encode(p, bits, mbs, 48000, bool(ms), trials) for p in s.pcm]
    decoded = [ob.decode(img)[0] for img in images]
    stats = np.zeros((len(images), ch, 4), dtype=np.int64)
    for i, (p, d) in enumerate(zip(s.pcm, decoded)):
        assert d.shape == p.shape
        e = p.astype(np.int64).T - d.astype(np.int64).T
        stats[i, :, 0], stats[i, :, 1], stats[i, :, 2], stats[i, :, 3] = (e * e).sum(axis=1), np.abs(e).sum(axis=1), np.abs(e).max(axis=1), e.shape[1]
    assert stats[..., 2].max() > 0 and (stats[:, :, 2] > 0).sum() > len(images) // 2  # the codec error is not zero
    for c in range(ch):  # a row's largest error on its last sample alone - the last sample of a unit tail - in every channel
        at_end = [i for i, (p, d) in enumerate(zip(s.pcm, decoded)) if len(p) >= 17 and
                  abs(int(p[-1, c]) - int(d[-1, c])) > np.abs(p[:-1, c].astype(np.int64) - d[:-1, c]).max()]
        assert at_end, ("no row whose largest error is its last sample's", c)
    return Expected(images, decoded, stats)


def assert_witnesses(ch, bits, ms, trials, seg, mbs, f32):
    """a launch of a neighbouring instantiation would give other bytes (module docstring)"""
    s, exp = samples(ch, bits, mbs, f32), expected(ch, bits, ms, trials, seg, mbs, f32)
    if ms:
        other = expected(ch, bits, 0, trials, seg, mbs, f32)
        assert sum(a != b for a, b in zip(exp.images, other.images)) > STREAMS // 2, "M/S and L/R images are the same"
    other = expected(ch, bits, ms, 0 if trials else 2, seg, mbs, f32)
    apart = 0
    for a, b in zip(exp.images, other.images):
        apart += any(a[o:o + s.block_size] != b[o:o + s.block_size] for o in range(31, len(a), s.block_size))
    assert apart > 0, "the trial search changes no block of the batch"
    other = expected(ch, bits, ms, trials, 0 if seg else 1, mbs, f32)
    assert any(a != b for a, b in zip(exp.images, other.images)), "segmented and serial images are the same"


# ---- one encoder launch ---------------------------------------------------------------------------------------------------------------
def _interleaved(pcm):
    """frames at odd offsets with garbage between them -> (flat int16, offsets)"""
    parts, offs, pos = [np.full(3, 77, dtype=np.int16)], [], 3
    for i, p in enumerate(pcm):
        offs.append(pos)
        parts += [p.reshape(-1), np.full(1 + i % 3, 77, dtype=np.int16)]
        pos += p.size + 1 + i % 3
    return np.concatenate(parts), np.array(offs, dtype=np.uint64)


def _chains(lengths, spb):
    return sum(len(so.segments(n, spb, *SEGMENTATION)) for n in lengths)


def run_encoder(engines, policy, cell, mbs):
    import torch
    bits, chf, ms, quad, trials_on, dual, ring, seg, inp, rec = cell.args
    ch, trials, f32 = chf or 3, 2 if trials_on else 0, inp == em.IN_PLANAR_F32
    label = (cell.kernel, cell.args, "max_block_size", mbs)
    s, exp = samples(ch, bits, mbs, f32), expected(ch, bits, ms, trials, seg, mbs, f32)
    assert_witnesses(ch, bits, ms, trials, seg, mbs, f32)
    engine = engines["ring" if ring else "plain"]
    mapping, lanes = "quad" if quad else "dense", "dual" if dual else "single"
    param = make_parameter(ch, bits, mbs, 48000, bool(ms), trials)
    n = len(s.lengths)
    table, total = image_table(engine, param, s.lengths, aligned=bool(ring))  # not aligned: no plan may take the ring
    assert [int(v) for v in table["data_size"]] == [len(img) for img in exp.images]
    ring_ok = int(all(int(o) % 64 == 0 for o in table["data_offset"]) and not seg)
    assert ring_ok == ring
    # the plan first: a record must not claim a kernel it did not run
    kind = "dense-ring" if ring else "quad-dual" if dual else "quad" if quad else "dense"
    planned = policy.encode(rec != em.REC_NONE, mapping, lanes, 2 if ring else 1, bits, ch, _chains(s.lengths, s.spb) if seg else n, trials,
                            s.block_size, ring_ok)
    assert planned == (kind, trials_on), (label, "planned", planned, "claimed", (kind, trials_on))
    segargs = SEGMENTATION if seg else (None, 0)
    data = torch.full((total,), IMG_CANARY, dtype=torch.uint8, device="cuda")
    assert data.data_ptr() % 64 == 0
    out_full = stats_full = None
    engine.set_mapping(mapping, lanes)
    try:
        if inp == em.IN_INTERLEAVED and rec == em.REC_NONE:
            flat, offs = _interleaved(s.pcm)
            table["pcm_offset"] = offs
            plan = engine.encode_plan(param, table, *segargs)
            try:
                plan.run(torch.from_numpy(flat).cuda(), data)
            finally:
                plan.close()
        else:
            # planar_layout (aad_encode_launch.hip.h): float32 rows, else mono int16 rows as interleaved frames, else int16 rows
            assert inp == (em.IN_PLANAR_F32 if f32 else em.IN_INTERLEAVED if ch == 1 else em.IN_PLANAR_I16)
            buf, offs, cs = lay_out(s.rows, ch, np.float32 if f32 else np.int16)
            assert cs > max(s.lengths)
            table["pcm_offset"] = offs
            x = torch.from_numpy(buf).cuda()
            in_dtype = torch.float32 if f32 else torch.int16
            if rec == em.REC_NONE:
                plan = engine.planar_encode_plan(param, table, cs, in_dtype, *segargs)
                try:
                    plan.run(x, data)
                finally:
                    plan.close()
            else:
                out_f32 = rec in (em.REC_F32, em.REC_F32_STATS)
                ocs, base = max(s.lengths) + 5, 8
                oss = ch * ocs + 13
                if rec != em.REC_STATS_ONLY:
                    out_full = (torch.full((base + n * oss + 11,), ROW_CANARY_F32, dtype=torch.int32, device="cuda").view(torch.float32) if out_f32
                                else torch.full((base + n * oss + 11,), ROW_CANARY_I16, dtype=torch.int16, device="cuda"))
                if rec >= em.REC_I16_STATS:
                    stats_full = torch.full((n * ch * 4 + 16,), STATS_CANARY, dtype=torch.int64, device="cuda")
                plan = engine.planar_reconstruct_plan(param, table, cs, in_dtype, torch.float32 if out_f32 else torch.int16, oss, ocs, *segargs)
                try:
                    plan.run(x, data, out_full[base:] if out_full is not None else None,
                             stats=stats_full[8:-8].view(n, ch, 4) if stats_full is not None else None)
                finally:
                    plan.close()
            torch.cuda.synchronize()
            assert np.array_equal(x.cpu().numpy().view(np.uint8), buf.view(np.uint8)), (label, "the input changed")
        torch.cuda.synchronize()
    finally:
        engine.set_mapping("auto", "dual")
    assert engine.last_error() == "", (label, engine.last_error())
    # the images, and the pattern around them
    got = data.cpu().numpy()
    want = np.full(total, IMG_CANARY, dtype=np.uint8)
    for d, img in zip(table, exp.images):
        want[int(d["data_offset"]):int(d["data_offset"]) + len(img)] = np.frombuffer(img, dtype=np.uint8)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(np.searchsorted(table["data_offset"].astype(np.int64), bad[0], side="right")) - 1
        pytest.fail("%r: image byte %d differs (stream %d of %d frames, byte %d of %d), %d bytes in all" % (
            label, bad[0], i, s.lengths[max(i, 0)], bad[0] - int(table["data_offset"][max(i, 0)]), len(exp.images[max(i, 0)]), bad.size))
    # the rows: the decode of the image, the pattern behind a stream's end and everywhere else
    if out_full is not None:
        ubits = np.uint32 if out_f32 else np.uint16
        o = out_full.cpu().numpy().view(ubits)
        want = np.full(o.size, ROW_CANARY_F32 if out_f32 else ROW_CANARY_I16, dtype=ubits)
        for i, d in enumerate(exp.decoded):
            for c in range(ch):
                at = base + i * oss + c * ocs
                v = d[:, c].astype(np.float32) / np.float32(32768) if out_f32 else np.ascontiguousarray(d[:, c])
                want[at:at + d.shape[0]] = v.view(ubits)
        bad = np.flatnonzero(o != want)
        if bad.size:
            e = int(bad[0]) - base
            pytest.fail("%r: row element %d differs (stream %d of %d frames, channel %d, frame %d): got %#x, want %#x, %d in all" % (
                label, bad[0], e // oss, s.lengths[min(max(e // oss, 0), n - 1)], e % oss // ocs, e % oss % ocs, o[bad[0]], want[bad[0]], bad.size))
    elif rec not in (em.REC_NONE, em.REC_STATS_ONLY):
        pytest.fail("%r: no rows were asked for" % (label,))
    if stats_full is not None:
        host = stats_full.cpu().numpy()
        assert (host[:8] == STATS_CANARY).all() and (host[-8:] == STATS_CANARY).all(), (label, "wrote outside its records")
        have = host[8:-8].reshape(n, ch, 4)
        assert np.array_equal(have, exp.stats), (label, "statistics differ from the sums over q(x) - decode at [stream, channel, field]",
                                                 np.argwhere(have != exp.stats)[:3].tolist(), have[have != exp.stats][:3].tolist(),
                                                 exp.stats[have != exp.stats][:3].tolist())
    RAN[(cell.kernel, cell.args)] += 1


ENCODE_GROUPS = em.encode_groups()


@pytest.mark.parametrize("group", ENCODE_GROUPS, ids=em.encode_group_id)
def test_encoder_kernels(engines, policy, group):
    mbs = (256, 301)[ENCODE_GROUPS.index(group) % 2]
    cells = em.encode_cells_of(group)
    assert 4 <= len(cells) <= 20
    for cell in cells:
        run_encoder(engines, policy, cell, mbs)


# ---- the decoders ----------------------------------------------------------------------------------------------------------------------
Geometry = collections.namedtuple("Geometry", "mbs block_size spb lengths layout")


def _decoder_geometry(cell, index):
    """the block size, lengths and table layout of a decoder record: 256 / 301 and the module's lengths wherever the plan takes them"""
    bits, chf, ms = cell.args[:3]
    ch = chf or 3
    fits = lambda mbs: True
    streams, layout, first, last = STREAMS, "ragged", (256, 301)[index % 2], 4400
    if cell.kernel == "decode_tiled_kernel":
        # decode_tiled_applicable: every block of a stream starts on a 16-byte piece of PCM (mono 2-bit: or 8 bytes past one) and, at
        # 3 bits, at the same offset of its code bytes inside a granule
        def fits(mbs):
            _, block_size, spb = ob.geometry(mbs, ch, bits)
            pcm_bytes = spb * ch * 2
            return (pcm_bytes % 16 == 0 or (bits == 2 and ch == 1 and pcm_bytes % 16 == 8)) and (bits != 3 or block_size % (64 * ch) == 0)
        layout = "aligned"
        if bits == 3 and ch == 1:  # 8 k + 4 samples a block: never whole pieces, so the plan takes one-block streams alone
            fits, layout = (lambda mbs: True), "aligned one-block"
    elif cell.kernel == "decode_blocks_kernel" and cell.args[4]:
        fits = lambda mbs: ob.geometry(mbs, ch, bits)[2] % 16 == 0  # whole 64-byte granules of stereo PCM from every block's first frame
        layout = "uniform"
    elif cell.kernel == "decode_split_kernel" and not cell.args[3]:
        fits = lambda mbs: ob.geometry(mbs, ch, bits)[2] - 4 > 2048  # kLdsResidualMax: the residual rows leave the LDS
        streams = 6
    mbs = next(m for m in range(first, last) if ob.geometry(m, ch, bits)[0] == 0 and fits(m))
    rc, block_size, spb = ob.geometry(mbs, ch, bits)
    lengths = [2 * spb + 13] * streams if layout == "uniform" else (block_lengths(spb)[3:] if streams == 6 else stream_lengths(spb))
    if layout == "aligned one-block":
        lengths, layout = [block_lengths(spb)[i % 6] for i in range(streams)], "aligned"
    return Geometry(mbs, block_size, spb, tuple(lengths), layout)


@functools.lru_cache(maxsize=None)
def decoder_streams(ch, bits, ms, mbs, lengths):
    """images of the oracle's encoder and their decodes"""
    src = synth_pcm(len(lengths), max(lengths), ch, seed=31 * ch + bits + mbs)
    images = [ob.encode(src[i, :n], bits, mbs, 48000, bool(ms), 0) for i, n in enumerate(lengths)]
    decoded = [ob.decode(img)[0] for img in images]
    assert any(d.any() for d in decoded)
    if ms:
        plain = [ob.encode(src[i, :n], bits, mbs, 48000, False, 0) for i, n in enumerate(lengths)]
        assert sum(a != b for a, b in zip(images, plain)) > len(lengths) // 2  # decoded as L/R these bytes give other samples
    return images, decoded


def _decoder_table(g, ch, sizes):
    """the stream table of a layout and the DecodeBatch it makes (decode_plan_init, aad_hip_engine.hip): ragged - odd PCM offsets,
    images at any byte; aligned - PCM on 16-byte boundaries, image pitches a multiple of the granule at one common phase; uniform -
    one pitch each, PCM base and pitch multiples of 64 bytes"""
    n = len(g.lengths)
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    granule = 64 if ch == 1 else 128
    pos_p, pos_d = {"ragged": (3, 5), "aligned": (8, 5), "uniform": (32, 64)}[g.layout]
    for i in range(n):
        d["pcm_offset"][i], d["data_offset"][i], d["data_size"][i], d["num_samples"][i] = pos_p, pos_d, sizes[i], g.lengths[i]
        if g.layout == "ragged":
            pos_p += g.lengths[i] * ch + 1 + i % 3
            pos_d += sizes[i] + 7 + i % 5
        elif g.layout == "aligned":
            pos_p += -(-(g.lengths[i] * ch + 1 + i % 3) // 8) * 8
            pos_d += -(-(sizes[i] + 7 + i % 5) // granule) * granule
        else:
            pos_p += -(-(g.lengths[i] * ch + 5) // 32) * 32
            pos_d += -(-(sizes[i] + 9) // 64) * 64
    blocks = sum(min(-(-g.lengths[i] // g.spb), -(-(sizes[i] - 31) // g.block_size)) for i in range(n))
    uniform = g.layout == "uniform"
    phase = 1 if g.block_size % granule == 0 else 2
    if any((int(o) - int(d["data_offset"][0])) % granule for o in d["data_offset"]):
        phase = 0
    stream_stores = uniform and ch == 2 and g.spb * 4 % 64 == 0  # the layout's base and pitch: 64 bytes above
    batch = (blocks, n, ch, 0, g.spb, g.block_size, all(int(o) * 2 % 16 == 0 for o in d["pcm_offset"]), 1, phase, stream_stores)
    return d, pos_p, pos_d, batch


def run_decoder(engines, policy, cell, index):
    import torch
    engine = engines["plain"]
    bits, chf, ms = cell.args[:3]
    ch = chf or 3
    g = _decoder_geometry(cell, index)
    label = (cell.kernel, cell.args, g.mbs, g.layout)
    images, decoded = decoder_streams(ch, bits, ms, g.mbs, g.lengths)
    d, n_pcm, n_dat, batch = _decoder_table(g, ch, [len(img) for img in images])
    batch = batch[:3] + (bits,) + batch[4:]
    role = SIMD_ROLE_OFF
    if cell.kernel == "decode_blocks_kernel":
        mapping, claim = ("quad-fused" if cell.args[3] else "dense"), ("quad-fused" if cell.args[3] else "dense", cell.args[4], False)
    elif cell.kernel == "decode_split_kernel":
        mapping, role = "quad", 1 if cell.args[4] else SIMD_ROLE_OFF
        claim = ("split-lds" if cell.args[3] else "split-scratch", 0, bool(cell.args[4]))
    else:
        mapping, claim = "dense-tiled", ("tiled", 0, False)
    planned = policy.decode(mapping, role, batch)
    assert planned == claim, (label, "planned", planned, "claimed", claim, "batch", batch)
    flat = np.full(n_dat + 256, 0xC3, dtype=np.uint8)
    for i, img in enumerate(images):
        flat[int(d["data_offset"][i]):int(d["data_offset"][i]) + len(img)] = np.frombuffer(img, dtype=np.uint8)
    d_img = torch.from_numpy(flat).cuda()
    pcm = torch.full((n_pcm + 64,), PCM_CANARY, dtype=torch.int16, device="cuda")
    assert pcm.data_ptr() % 64 == 0
    engine.set_mapping(mapping)
    engine.set_simd_role(None if role == SIMD_ROLE_OFF else role)
    try:
        plan = engine.decode_plan(parse_header(images[0][:31]), d, True)
        try:
            plan.run(d_img, pcm)
            torch.cuda.synchronize()
        finally:
            plan.close()
    finally:
        engine.set_mapping("auto")
        engine.set_simd_role(None)
    assert engine.last_error() == "", (label, engine.last_error())
    want = np.full(n_pcm + 64, PCM_CANARY, dtype=np.int16)
    for i, dec in enumerate(decoded):
        want[int(d["pcm_offset"][i]):int(d["pcm_offset"][i]) + dec.size] = dec.reshape(-1)
    got = pcm.cpu().numpy()
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(np.searchsorted(d["pcm_offset"].astype(np.int64), bad[0], side="right")) - 1
        pytest.fail("%r: PCM element %d differs (stream %d of %d frames, element %d): got %d, want %d, %d in all" % (
            label, bad[0], i, g.lengths[max(i, 0)], bad[0] - int(d["pcm_offset"][max(i, 0)]), got[bad[0]], want[bad[0]], bad.size))
    assert np.array_equal(d_img.cpu().numpy(), flat), (label, "the images changed")
    RAN[(cell.kernel, cell.args)] += 1


DECODE_GROUPS = em.decode_groups()


@pytest.mark.parametrize("group", DECODE_GROUPS, ids=em.decode_group_id)
def test_decoder_kernels(engines, policy, group):
    for cell in em.decode_cells_of(group):
        run_decoder(engines, policy, cell, DECODE_GROUPS.index(group))


def test_zz_every_record_ran(capsys):
    """the closing case: every reachable encoder and decoder record was launched and compared once (run after the cases above; a
    run of a part of this file fails here)"""
    cells = em.matrix_cells()
    per_kernel, table = collections.Counter(k for k, _ in RAN), collections.Counter(c.kernel for c in cells)
    with capsys.disabled():
        print("\nrecords run per kernel:", dict(per_kernel), "of", dict(table))
    missing = sorted((c.kernel, c.args) for c in cells if RAN[(c.kernel, c.args)] != 1)
    assert not missing, ("records not run exactly once", len(missing), missing[:8])
    assert per_kernel == table and sum(RAN.values()) == len(cells) == 1210
    assert dict(table) == {k: em.COUNTS[k] for k in table}
