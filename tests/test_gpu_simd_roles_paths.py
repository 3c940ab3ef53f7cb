"""Every kernel and host path that AAD_HIP_OPTION_SIMD_ROLE changes, against the CPU oracle (tests/test_gpu_simd_roles.py covers
encode_uniform / decode_uniform on equal-length int16 streams without trials; this module the rest).

The option sits on the context, so plan_encode / plan_decode (aad_launch_policy.h) apply it to every run of that context.  Under a
role every quad encoder without the dual search - encode_streams_kernel<QUAD, !DUAL>, all IN (interleaved, planar int16 / float32),
REC (none, rows, rows + statistics, statistics only), SEG and TRIALS variants - runs four-wave workgroups with an elected worker
wave, and the split decoder runs its ROLE instantiations (elected recurrence wave, block-sized residual rows in dynamic LDS, the
scan on one SIMD pair).

Bar: bit-exact.  The expected value is always the oracle's (oracle_binding.encode / decode, segment_oracle, numpy int64 sums, the
compiled reference's hashes of tests/golden/bitstream_fuzz.json); in addition every check holds the role-on result to the role-off
result of the same engine.  Images as bytes, int16 and float32 rows ==, int64 statistics ==.  The one exception: the fp64 reordered
sums of the host reconstruct modes keep tests/test_gpu_reconstruct.py's bar (STATS_RTOL, == on the maximum and the printed line).

Shapes: block size 256; 1, 9 and 17 streams (a partial quad wave, two workgroups, a ragged last workgroup) whose lengths are ragged
within a batch - 1, 4, 5, 20, spb, spb + 1, 2 spb + 19 frames, cycled."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bitstream_fuzz as bf
import crafted_pcm as cp
import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import LANE_STATE_DTYPE, STREAM_DESC_DTYPE, make_parameter
from aad_amd.synth import synth_pcm
from test_gpu_bitstream_fuzz import BATCHES, _same_format_batch
from test_gpu_crafted_pcm import DOZEN, LONG_2BIT
from test_gpu_planar_encode import make_rows, q
from test_gpu_planar_stats import expected_stats
from test_gpu_reconstruct import STATS_RTOL, _as_tuple
from window_oracle import window_expected

pytestmark = pytest.mark.gpu

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MBS = 256
STREAMS = (1, 9, 17)
ROLES = [None, 0, 1, 2, 3]
FORMATS = [(ch, bits, ms) for ch, ms in ((1, False), (2, False), (2, True)) for bits in (4, 3, 2)]
PCM_CANARY = 0x5A5A


def role_id(r):
    return "off" if r is None else "simd%d" % r


def format_id(f):
    return "%dch%db%s" % (f[0], f[1], "ms" if f[2] else "")


by_role = pytest.mark.parametrize("role", ROLES, ids=role_id)
by_format = pytest.mark.parametrize("fmt", FORMATS, ids=format_id)


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def restored(engine):
    """whatever a test sets on the context - role, mapping, trial lanes, tile size - is put back when it leaves"""
    try:
        yield engine
    finally:
        engine.set_simd_role(None)
        engine.set_mapping("auto", "dual")
        engine.set_tile_kbytes(0)


def off_and_on(engine, role, run):
    """-> (run() with the role off, run() under `role`); role None: the role-off result twice"""
    engine.set_simd_role(None)
    off = run()
    if role is None:
        return off, off
    engine.set_simd_role(role)
    try:
        return off, run()
    finally:
        engine.set_simd_role(None)


def spb_of(ch, bits, mbs=MBS):
    rc, _, spb = ob.geometry(mbs, ch, bits)
    assert rc == 0
    return spb


def ragged_lengths(spb, streams=max(STREAMS)):
    base = [1, 4, 5, 20, spb, spb + 1, 2 * spb + 19]
    return [base[i % len(base)] for i in range(streams)]


# float32 samples on rounding ties of x * 32768 (to even: 0.5 -> 0, 1.5 -> 2, -0.5 -> -0, -2.5 -> -2, 2.5 -> 2) and past both rails
F32_EDGES = np.array([0.5, 1.5, -0.5, -2.5, 2.5, 32767.5, 32768.0, 98304.0, -32768.5, -32769.0, -229376.0, 32766.5],
                     dtype=np.float64) / 32768.0

_rows = {}


def input_rows(fmt, dtype):
    """the seventeen ragged streams of a format as [C, n] rows of the sample type, made once; float32 rows carry the ties and the
    values past full scale of test_gpu_planar_encode.make_rows and, from 20 frames on, F32_EDGES on every channel"""
    key = (fmt, np.dtype(dtype).name)
    if key not in _rows:
        ch, bits, ms = fmt
        lens = ragged_lengths(spb_of(ch, bits))
        rows = make_rows(np.random.default_rng(100 * ch + bits), ch, lens, dtype, seed=7 * ch + bits + ms)
        if dtype == np.float32:
            for r in rows:
                if r.shape[1] >= 20:
                    r[:, 6:6 + len(F32_EDGES)] = F32_EDGES.astype(np.float32)
            got = q(rows[3])[0, 6:6 + len(F32_EDGES)].tolist()
            assert got == [0, 2, 0, -2, 2, 32767, 32767, 32767, -32768, -32768, -32768, 32766], got
        _rows[key] = rows
    return _rows[key]


_wanted = {}


def wanted(fmt, dtype, trials, seg=None):
    """per stream (oracle image, oracle decode as [C, n] int16) of input_rows, computed once"""
    key = (fmt, np.dtype(dtype).name, trials, seg)
    if key not in _wanted:
        ch, bits, ms = fmt
        out = []
        for r in (input_rows(fmt, dtype) if seg is None else segment_rows(fmt, dtype)):
            p = np.ascontiguousarray(q(r).T)
            img = ob.encode(p, bits, MBS, 48000, ms, trials) if seg is None else \
                so.segmented_encode(p, bits, seg[0], seg[1], MBS, ms=ms, trials=trials)
            out.append((img, np.ascontiguousarray(ob.decode(img)[0].T)))
        _wanted[key] = out
    return _wanted[key]


def planar_tensor(torch, rows, view):
    """rows -> cuda tensor [N, C, T], T the longest row, garbage past every row's end.  view: a slice of a bigger tensor, its channel
    stride above T (stride(-1) == 1 still)"""
    n, ch, t = len(rows), rows[0].shape[0], max(r.shape[1] for r in rows)
    shape = (n + 2, ch, t + 7) if view else (n, ch, t)
    host = np.full(shape, 12345, dtype=np.int16) if rows[0].dtype == np.int16 else np.full(shape, 9.25, dtype=np.float32)
    s0, t0 = (1, 3) if view else (0, 0)
    for i, r in enumerate(rows):
        host[s0 + i, :, t0:t0 + r.shape[1]] = r
    x = torch.from_numpy(host).cuda()
    x = x[1:n + 1, :, 3:3 + t] if view else x
    assert tuple(x.shape) == (n, ch, t) and x.stride(-1) == 1 and (not view or (x.stride(1) > t and x.stride(0) > ch * t))
    return x


def check_images(label, images, sizes, want):
    for i, (img, _) in enumerate(want):
        assert int(sizes[i]) == len(img), (label, i, int(sizes[i]), len(img))
        assert bytes(images[i, :len(img)]) == img, cp.describe_mismatch("%s, stream %d" % (label, i), images[i, :len(img)], img)


def check_rows(label, y, want, out_dtype):
    """y: [N, C, T] int16 or float32 rows == the oracle's decode (float32: / 32768, which is exact), zero past each stream's end"""
    exp = np.zeros(y.shape, dtype=np.int16)
    for i, (_, dec) in enumerate(want):
        exp[i, :, :dec.shape[1]] = dec
    if out_dtype == np.float32:
        exp = exp.astype(np.float32) / np.float32(32768.0)
    assert y.dtype == exp.dtype
    bad = np.argwhere(y != exp)
    assert bad.size == 0, (label, "rows differ first at [stream, channel, frame]", bad[0].tolist(), len(bad))


def same(label, off, on):
    """role-on == role-off, element for element, over whatever a run returned (numpy arrays, lists of them, bytes, ints)"""
    if isinstance(off, (list, tuple)):
        assert len(off) == len(on), label
        for k, (a, b) in enumerate(zip(off, on)):
            same((label, k), a, b)
    elif isinstance(off, np.ndarray):
        assert off.dtype == on.dtype and off.shape == on.shape and off.tobytes() == on.tobytes(), (label, "role on differs from role off")
    else:
        assert off == on, (label, "role on differs from role off")


# ---- 1. encoder instantiations under a role ------------------------------------------------------------------------------------

@by_format
@by_role
def test_planar_encode(engine, role, fmt):
    """Engine.encode_planar: encode_streams_kernel<QUAD, IN = planar int16 / planar float32>, non-uniform table, contiguous and as a
    view (channel stride above T, a slice of a bigger tensor), float32 ties and rails: the oracle's image of q(x)"""
    import torch
    ch, bits, ms = fmt
    param = make_parameter(ch, bits, MBS, 48000, ms, 0)
    with restored(engine):
        for dtype in (np.int16, np.float32):
            rows, want = input_rows(fmt, dtype), wanted(fmt, dtype, 0)
            for streams in STREAMS:
                for view in (False, True):
                    x = planar_tensor(torch, rows[:streams], view)
                    lens = [r.shape[1] for r in rows[:streams]]

                    def run():
                        out, sizes = engine.encode_planar(x, param, num_samples=lens)
                        torch.cuda.synchronize()
                        return [out.cpu().numpy(), sizes]
                    label = ("encode_planar", role_id(role), fmt, np.dtype(dtype).name, streams, view)
                    off, on = off_and_on(engine, role, run)
                    for res in (off, on):
                        check_images(label, res[0], res[1], want[:streams])
                    same(label, off, on)


REC_KINDS = ["i16", "f32", "i16+stats", "f32+stats", "stats"]


def filled_stats(engine, torch, x, param, lens, out_dtype, kw):
    """The statistics of a planar reconstruct run once more, through a plan, into a table filled with a pattern first (out_dtype
    None: statistics only, else with rows of that type).  Engine.reconstruct_planar / codec_error hand the kernel a torch.empty
    table: a block that an earlier run has just freed comes back holding that run's (right) records, so records the kernel failed
    to write would read back correct there."""
    n, ch, t = (int(v) for v in x.shape)
    stride = -(-max(engine.encoded_size(param, int(v)) for v in lens) // 64) * 64
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    d["pcm_offset"], d["data_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(x.stride(0)), np.arange(n, dtype=np.uint64) * np.uint64(stride)
    d["data_size"], d["num_samples"] = stride, lens
    images = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    table = torch.full((n, ch, 4), -7, dtype=torch.int64, device="cuda")
    y = None if out_dtype is None else torch.zeros((n, ch, t), dtype=out_dtype, device="cuda")
    plan = engine.planar_reconstruct_plan(param, d, x.stride(1), x.dtype, out_dtype or x.dtype, ch * t, t, kw.get("segment_blocks"),
                                          kw.get("warmup_blocks", 0))
    try:
        plan.run(x, images, y, None, stats=table)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return table.cpu().numpy()


def reconstruct_run(engine, torch, x, param, lens, kind, **kw):
    """one planar reconstruct run of a REC kind -> dict of numpy results (rows, images, sizes, stats as the kind has them; a kind with
    statistics, run without a state table, also "stats into a filled table": filled_stats)"""
    if kind == "stats":
        stats = engine.codec_error(x, param, num_samples=lens, **kw)
        torch.cuda.synchronize()
        out = {"stats": stats.cpu().numpy()}
        if "state" not in kw:
            out["stats into a filled table"] = filled_stats(engine, torch, x, param, lens, None, kw)
        return out
    out_dtype = torch.float32 if kind.startswith("f32") else torch.int16
    res = engine.reconstruct_planar(x, param, num_samples=lens, dtype=out_dtype, return_images=True,
                                    return_stats=kind.endswith("+stats"), **kw)
    torch.cuda.synchronize()
    out = {"rows": res[0].cpu().numpy(), "images": res[1].cpu().numpy(), "sizes": res[2]}
    if kind.endswith("+stats"):
        out["stats"] = res[3].cpu().numpy()
        if "state" not in kw:
            out["stats into a filled table"] = filled_stats(engine, torch, x, param, lens, out_dtype, kw)
    return out


def check_reconstruct(label, res, rows, want, kind):
    if "images" in res:
        check_images(label, res["images"], res["sizes"], want)
        check_rows(label, res["rows"], want, np.float32 if kind.startswith("f32") else np.int16)
    for key in ("stats", "stats into a filled table"):
        if key in res:
            exp = expected_stats(rows, [dec for _, dec in want])
            assert res[key].dtype == np.int64 and np.array_equal(res[key], exp), (label, key, np.argwhere(res[key] != exp)[:3].tolist())


@by_format
@by_role
def test_planar_reconstruct(engine, role, fmt):
    """Engine.reconstruct_planar / codec_error: encode_streams_kernel<QUAD, IN planar, REC 1..5> - int16 rows, float32 rows, each
    with statistics, statistics only - without trials and with two (plan_reconstruct_encode forces single trial lanes: the TRIALS
    quad kernel under a role).  Images == ob.encode, rows == ob.decode, statistics == the integer sums of q(x) - decoded."""
    import torch
    ch, bits, ms = fmt
    with restored(engine):
        for trials in (0, 2):
            param = make_parameter(ch, bits, MBS, 48000, ms, trials)
            for dtype in (np.int16, np.float32):
                rows, want = input_rows(fmt, dtype), wanted(fmt, dtype, trials)
                for streams in STREAMS:
                    x = planar_tensor(torch, rows[:streams], view=streams == 9)
                    lens = [r.shape[1] for r in rows[:streams]]
                    for kind in REC_KINDS:
                        label = ("reconstruct_planar", role_id(role), fmt, trials, np.dtype(dtype).name, streams, kind)
                        off, on = off_and_on(engine, role, lambda: reconstruct_run(engine, torch, x, param, lens, kind))
                        for res in (off, on):
                            check_reconstruct(label, res, rows[:streams], want[:streams], kind)
                        same(label, sorted(off.items()), sorted(on.items()))


def ragged_encode(engine, torch, pcms, param, state=None, seg=None):
    """a device-resident encode plan over a non-uniform table (odd PCM offsets, images 64 bytes apart and more) -> [bytes]"""
    ch = param.num_channels
    d = np.zeros(len(pcms), dtype=STREAM_DESC_DTYPE)
    pos_p, pos_d, sizes, parts = 3, 0, [], [np.zeros(3, dtype=np.int16)]
    for i, p in enumerate(pcms):
        size = engine.encoded_size(param, p.shape[0])
        sizes.append(size)
        d["pcm_offset"][i], d["data_offset"][i], d["data_size"][i], d["num_samples"][i] = pos_p, pos_d, size, p.shape[0]
        parts += [p.reshape(-1), np.full(1 + i % 3, 77, dtype=np.int16)]
        pos_p += p.shape[0] * ch + 1 + i % 3
        pos_d += -(-size // 64) * 64 + 64 * (i % 2)
    d_pcm = torch.from_numpy(np.concatenate(parts)).cuda()
    d_img = torch.zeros(pos_d + 64, dtype=torch.uint8, device="cuda")
    plan = engine.encode_plan(param, d, *(seg or (None, 0)))
    try:
        plan.run(d_pcm, d_img, state)
        torch.cuda.synchronize()
    finally:
        plan.close()
    img = d_img.cpu().numpy()
    return [img[int(d["data_offset"][i]):int(d["data_offset"][i]) + sizes[i]].tobytes() for i in range(len(pcms))]


def ragged_decode(engine, torch, images, sizes=None, fill=PCM_CANARY):
    """a device-resident decode plan over a non-uniform table: images of one format at odd byte offsets, data_size = sizes (default:
    all of each image), PCM runs with gaps -> [int16 [n, C]]; nothing outside the runs may be written"""
    from aad_amd.engine import parse_header
    hd = parse_header(images[0][:31])
    ch = hd.num_channels
    sizes = [len(b) for b in images] if sizes is None else sizes
    d = np.zeros(len(images), dtype=STREAM_DESC_DTYPE)
    pos_p, pos_d = 0, 5
    for i, b in enumerate(images):
        n = parse_header(b[:31]).num_samples
        d["pcm_offset"][i], d["data_offset"][i], d["data_size"][i], d["num_samples"][i] = pos_p, pos_d, sizes[i], n
        pos_p += n * ch + 3 + i % 2
        pos_d += len(b) + 7 + i % 5
    flat = np.zeros(pos_d + 16, dtype=np.uint8)
    for i, b in enumerate(images):
        flat[int(d["data_offset"][i]):int(d["data_offset"][i]) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    d_img = torch.from_numpy(flat).cuda()
    out = torch.full((pos_p + 32,), fill, dtype=torch.int16, device="cuda")
    plan = engine.decode_plan(hd, d, True)
    try:
        plan.run(d_img, out)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert engine.last_error() == "", engine.last_error()
    host = out.cpu().numpy()
    mask = np.ones(host.size, dtype=bool)
    got = []
    for i in range(len(images)):
        o, n = int(d["pcm_offset"][i]), int(d["num_samples"][i]) * ch
        mask[o:o + n] = False
        got.append(host[o:o + n].reshape(-1, ch).copy())
    assert (host[mask] == np.int16(fill)).all(), "a sample outside the streams' runs was written"
    return got


_interleaved = {}


def interleaved_case(fmt, trials):
    """-> (ragged pcms [n, C], their oracle images and decodes, a uniform batch [17, 2 spb + 19, C] with its images and decodes)"""
    key = (fmt, trials)
    if key not in _interleaved:
        ch, bits, ms = fmt
        pcms = [np.ascontiguousarray(r.T) for r in input_rows(fmt, np.int16)]
        uni = synth_pcm(max(STREAMS), 2 * spb_of(ch, bits) + 19, ch, seed=300 + 10 * ch + bits, kind="music")
        uni[1::3] = synth_pcm(len(uni[1::3]), uni.shape[1], ch, seed=301 + bits, kind="noise")
        enc = lambda p: ob.encode(p, bits, MBS, 48000, ms, trials)
        r_img, u_img = [enc(p) for p in pcms], [enc(p) for p in uni]
        _interleaved[key] = (pcms, r_img, [ob.decode(i)[0] for i in r_img], uni, u_img, [ob.decode(i)[0] for i in u_img])
    return _interleaved[key]


@by_format
@by_role
def test_interleaved_trial_lanes(engine, role, fmt):
    """encode_uniform and a ragged EncodePlan with one and two trials, once per trial-lane setting: single lanes under a role are
    encode_streams_kernel<QUAD, TRIALS, !DUAL> with the elected worker wave; dual lanes keep the QuadDual launch (plan_encode gives it
    no role) while the decode of the same context still takes one.  Images == ob.encode, decodes == ob.decode."""
    import torch
    ch, bits, ms = fmt
    with restored(engine):
        for lanes in ("single", "dual"):
            engine.set_mapping("auto", lanes)
            for trials in (1, 2):
                param = make_parameter(ch, bits, MBS, 48000, ms, trials)
                pcms, r_img, r_dec, uni, u_img, u_dec = interleaved_case(fmt, trials)
                for streams in STREAMS:
                    d_uni = torch.from_numpy(uni[:streams]).cuda()

                    def run():
                        d_img, size = engine.encode_uniform(d_uni, param)
                        d_dec, _ = engine.decode_uniform(d_img, size)
                        torch.cuda.synchronize()
                        images = ragged_encode(engine, torch, pcms[:streams], param)
                        return [d_img.cpu().numpy()[:, :size], d_dec.cpu().numpy(), images, ragged_decode(engine, torch, images)]
                    label = ("trial lanes", lanes, role_id(role), fmt, trials, streams)
                    off, on = off_and_on(engine, role, run)
                    for res in (off, on):
                        for s in range(streams):
                            assert bytes(res[0][s]) == u_img[s], cp.describe_mismatch("%s uniform %d" % (label, s), res[0][s], u_img[s])
                            assert np.array_equal(res[1][s], u_dec[s]), (label, "uniform decode", s)
                            assert res[2][s] == r_img[s], cp.describe_mismatch("%s ragged %d" % (label, s), res[2][s], r_img[s])
                            assert np.array_equal(res[3][s], r_dec[s]), (label, "ragged decode", s)
                    same(label, off, on)


SEG = (2, 1)  # segment_blocks, warmup_blocks
_seg_rows = {}


def segment_rows(fmt, dtype):
    """seventeen 7-block streams as [C, n] rows: last blocks of spb, 1, 5, 20 and spb - 1 frames; float32 = int16 / 32768 (exact)"""
    key = (fmt, np.dtype(dtype).name)
    if key not in _seg_rows:
        ch, bits, _ = fmt
        spb = spb_of(ch, bits)
        lens = [6 * spb + (spb, 1, 5, 20, spb - 1)[i % 5] for i in range(max(STREAMS))]
        src = synth_pcm(len(lens), 7 * spb, ch, seed=900 + 10 * ch + bits, kind="music")
        rows = [np.ascontiguousarray(src[i, :n].T) for i, n in enumerate(lens)]
        _seg_rows[key] = rows if dtype == np.int16 else [r.astype(np.float32) / np.float32(32768.0) for r in rows]
    return _seg_rows[key]


_seg_uniform = {}


def segment_uniform(fmt, trials):
    """seventeen equal-length 7-block streams (the last block holds 19 frames) for encode_uniform, with the definition's images and
    their decodes, computed once -> (pcm [17, 6 spb + 19, C], [image], [decode [n, C]])"""
    key = (fmt, trials)
    if key not in _seg_uniform:
        ch, bits, ms = fmt
        pcm = synth_pcm(max(STREAMS), 6 * spb_of(ch, bits) + 19, ch, seed=950 + 10 * ch + bits, kind="music")
        pcm[2::3] = synth_pcm(len(pcm[2::3]), pcm.shape[1], ch, seed=951 + bits, kind="noise")
        images = [so.segmented_encode(p, bits, SEG[0], SEG[1], MBS, ms=ms, trials=trials) for p in pcm]
        _seg_uniform[key] = (pcm, images, [ob.decode(i)[0] for i in images])
    return _seg_uniform[key]


@by_format
@by_role
def test_segmented(engine, role, fmt):
    """segment_blocks = 2, warmup_blocks = 1 on 7-block streams (four chains a stream: 4, 36 and 68 chains x channels recurrences):
    encode_uniform over 1, 9 and 17 equal-length streams and a ragged EncodePlan over the streams of segment_rows
    (encode_streams_kernel<QUAD, SEG>, without trials and - single lanes - with two), encode_planar (SEG, IN planar) and
    reconstruct_planar with statistics (SEG, REC) == tests/segment_oracle.py's image, its decode and the integer sums"""
    import torch
    ch, bits, ms = fmt
    with restored(engine):
        engine.set_mapping("auto", "single")
        for trials in (0, 2):
            param = make_parameter(ch, bits, MBS, 48000, ms, trials)
            uni, u_img, u_dec = segment_uniform(fmt, trials)
            rows16, want16 = segment_rows(fmt, np.int16), wanted(fmt, np.int16, trials, SEG)
            for streams in STREAMS:
                d_pcm = torch.from_numpy(uni[:streams]).cuda()
                pcms = [np.ascontiguousarray(r.T) for r in rows16[:streams]]

                def run_interleaved():
                    d_img, size = engine.encode_uniform(d_pcm, param, segment_blocks=SEG[0], warmup_blocks=SEG[1])
                    d_dec, _ = engine.decode_uniform(d_img, size)
                    torch.cuda.synchronize()
                    return [d_img.cpu().numpy()[:, :size], d_dec.cpu().numpy(), ragged_encode(engine, torch, pcms, param, seg=SEG)]
                label = ("segmented interleaved", role_id(role), fmt, trials, streams)
                off, on = off_and_on(engine, role, run_interleaved)
                for res in (off, on):
                    assert len(res[0]) == len(res[2]) == streams
                    for i in range(streams):
                        assert bytes(res[0][i]) == u_img[i], cp.describe_mismatch("%s uniform stream %d" % (label, i), res[0][i], u_img[i])
                        assert np.array_equal(res[1][i], u_dec[i]), (label, "decode", i)
                        assert res[2][i] == want16[i][0], cp.describe_mismatch("%s ragged stream %d" % (label, i), res[2][i], want16[i][0])
                same(label, off, on)
                if trials and streams != 9:
                    continue  # the planar forms with trials: once
                for dtype in (np.int16, np.float32):
                    rows, want = segment_rows(fmt, dtype)[:streams], wanted(fmt, dtype, trials, SEG)[:streams]
                    x = planar_tensor(torch, rows, view=dtype == np.float32)
                    lens = [r.shape[1] for r in rows]

                    def run_planar():
                        out, sizes = engine.encode_planar(x, param, num_samples=lens, segment_blocks=SEG[0], warmup_blocks=SEG[1])
                        torch.cuda.synchronize()
                        kind = "f32+stats" if dtype == np.float32 else "i16+stats"
                        rec = reconstruct_run(engine, torch, x, param, lens, kind, segment_blocks=SEG[0], warmup_blocks=SEG[1])
                        err = reconstruct_run(engine, torch, x, param, lens, "stats", segment_blocks=SEG[0], warmup_blocks=SEG[1])
                        return [out.cpu().numpy(), sizes, sorted(rec.items()), sorted(err.items())]
                    label = ("segmented planar", role_id(role), fmt, trials, np.dtype(dtype).name, streams)
                    off, on = off_and_on(engine, role, run_planar)
                    for res in (off, on):
                        check_images(label, res[0], res[1], want)
                        check_reconstruct(label, dict(res[2]), rows, want, "f32+stats" if dtype == np.float32 else "i16+stats")
                        check_reconstruct(label, dict(res[3]), rows, want, "stats")
                    same(label, off, on)


_state_cases = {}


def state_case(fmt, uniform=False):
    """Seventeen streams cut at a block boundary (after one or two blocks; uniform - encode_uniform's equal lengths - after one, with
    2 spb + 19 frames behind it: two full blocks and a short one of coded samples on the carried state) into two calls.  Without trials and with the step index
    carried (not reset between the calls) the two calls' bodies are the one-shot image's body and the state after the second call is
    the one-shot encoder's: asserted here on the oracle itself.  -> (first halves, second halves [n, C], images of call 1, images of
    call 2, final lanes per stream)"""
    if (fmt, uniform) not in _state_cases:
        ch, bits, ms = fmt
        spb = spb_of(ch, bits)
        tails = [2 * spb + 19] * max(STREAMS) if uniform else ragged_lengths(spb)
        firsts, seconds, img1, img2, final = [], [], [], [], []
        for i, tail in enumerate(tails):
            n1 = spb if uniform else spb * (1 + i % 2)
            pcm = synth_pcm(1, n1 + tail, ch, seed=4000 + 17 * i + bits + 500 * uniform, kind=("music", "noise")[i % 2])[0]
            one_shot_lanes, lanes = ob.fresh_lanes(ch), ob.fresh_lanes(ch)
            whole = ob.encode(pcm, bits, MBS, 48000, ms, 0, lanes=one_shot_lanes)
            a = ob.encode(pcm[:n1], bits, MBS, 48000, ms, 0, lanes=lanes)
            b = ob.encode(pcm[n1:], bits, MBS, 48000, ms, 0, lanes=lanes, reset_idx=False)
            assert a[31:] + b[31:] == whole[31:]
            for c in range(ch):
                assert (list(lanes[c].w), list(lanes[c].h), lanes[c].idx, lanes[c].qerr) == \
                    (list(one_shot_lanes[c].w), list(one_shot_lanes[c].h), one_shot_lanes[c].idx, one_shot_lanes[c].qerr)
            firsts.append(pcm[:n1])
            seconds.append(pcm[n1:])
            img1.append(a)
            img2.append(b)
            final.append(one_shot_lanes)
        _state_cases[(fmt, uniform)] = (firsts, seconds, img1, img2, final)
    return _state_cases[(fmt, uniform)]


def check_state(label, records, final, ch):
    """records: LANE_STATE_DTYPE [streams * C] == the oracle's lanes"""
    for i, lanes in enumerate(final):
        for c in range(ch):
            r = records[i * ch + c]
            got = (list(r["weight"]), list(r["history"]), int(r["stepsize_index"]), int(r["quantize_error"]))
            exp = (list(lanes[c].w), list(lanes[c].h), lanes[c].idx, lanes[c].qerr)
            assert got == exp, (label, "state of stream %d channel %d" % (i, c), got, exp)


STATE_CALLERS = ["encode_uniform", "encode_planar_i16", "encode_planar_f32", "reconstruct_planar", "codec_error", "encode_host",
                 "encode_plan"]


def state_two_calls(engine, torch, caller, fmt, streams, roles):
    """encode the streams of state_case as two successive calls through `caller`, call k under roles[k] -> (images of call 1, images
    of call 2, LANE_STATE_DTYPE records after call 2, extra results of call 2)"""
    ch, bits, ms = fmt
    param = make_parameter(ch, bits, MBS, 48000, ms, 0)
    firsts, seconds = (h[:streams] for h in state_case(fmt, uniform=caller == "encode_uniform")[:2])
    n = len(firsts)
    host_state = np.zeros(n * ch, dtype=LANE_STATE_DTYPE)
    state = torch.zeros((n * ch, 10), dtype=torch.int32, device="cuda")
    images, extra = [], None
    for k, half in enumerate((firsts, seconds)):
        engine.set_simd_role(roles[k])
        lens = [p.shape[0] for p in half]
        if caller == "encode_uniform":
            d_img, size = engine.encode_uniform(torch.from_numpy(np.stack(half)).cuda(), param, state=state)
            torch.cuda.synchronize()
            images.append([bytes(r[:size]) for r in d_img.cpu().numpy()])
        elif caller == "encode_plan":
            images.append(ragged_encode(engine, torch, half, param, state=state))
        elif caller == "encode_host":
            images.append(engine.encode_host(half, param, state=host_state))
        else:
            rows = [np.ascontiguousarray(p.T) for p in half]
            if caller == "encode_planar_f32":
                rows = [r.astype(np.float32) / np.float32(32768.0) for r in rows]
            x = planar_tensor(torch, rows, view=k == 1)
            if caller.startswith("encode_planar"):
                out, sizes = engine.encode_planar(x, param, num_samples=lens, state=state)
                torch.cuda.synchronize()
                out = out.cpu().numpy()
                images.append([bytes(out[i, :sizes[i]]) for i in range(n)])
            elif caller == "reconstruct_planar":
                res = reconstruct_run(engine, torch, x, param, lens, "i16+stats", state=state)
                images.append([bytes(res["images"][i, :res["sizes"][i]]) for i in range(n)])
                extra = [res["rows"], res["stats"]]
            else:  # codec_error: no image leaves the call; its statistics and the state do
                res = reconstruct_run(engine, torch, x, param, lens, "stats", state=state)
                images.append(None)
                extra = [res["stats"]]
    engine.set_simd_role(None)
    records = host_state if caller == "encode_host" else state.cpu().numpy().view(LANE_STATE_DTYPE).reshape(-1)
    return images[0], images[1], records.copy(), extra


@pytest.mark.parametrize("caller", STATE_CALLERS)
@by_format
@by_role
def test_state_in_and_out(engine, role, fmt, caller):
    """Every caller that hands a state table to the encoders (encode_uniform, encode_planar from int16 and float32, reconstruct_planar,
    codec_error, encode_host, a ragged EncodePlan.run): a stream as two successive calls, the first under the role and the second
    without and the reverse.  Both calls' images == the oracle's successive encodes - whose bodies together are the one-shot image's
    body (state_case) - and the records after the second call == the oracle's final lanes, every field."""
    import torch
    ch, bits, ms = fmt
    firsts, seconds, img1, img2, final = state_case(fmt, uniform=caller == "encode_uniform")
    with restored(engine):
        for streams in STREAMS:
            base = state_two_calls(engine, torch, caller, fmt, streams, (None, None))
            for roles in ([(role, None), (None, role)] if role is not None else [(None, None)]):
                label = ("state", caller, fmt, streams, tuple(role_id(r) for r in roles))
                got = state_two_calls(engine, torch, caller, fmt, streams, roles)
                pick = list(range(streams))
                for k, i in enumerate(pick):
                    if got[0] is not None:
                        assert got[0][k] == img1[i], cp.describe_mismatch("%s call 1 stream %d" % (label, i), got[0][k], img1[i])
                    if got[1] is not None:
                        assert got[1][k] == img2[i], cp.describe_mismatch("%s call 2 stream %d" % (label, i), got[1][k], img2[i])
                check_state(label, got[2], [final[i] for i in pick], ch)
                if got[3] is not None:  # call 2's rows and statistics: the decode of call 2's image (a block header holds the state)
                    want = [(img2[i], np.ascontiguousarray(ob.decode(img2[i])[0].T)) for i in pick]
                    rows = [np.ascontiguousarray(seconds[i].T) for i in pick]
                    if len(got[3]) == 2:
                        check_rows(label, got[3][0], want, np.int16)
                    check_reconstruct(label, {"stats": got[3][-1]}, rows, want, "stats")
                same(label, [v for v in base if v is not None], [v for v in got if v is not None])


@by_format
@by_role
def test_window_reconstruct(engine, role, fmt):
    """Engine.reconstruct_windows / codec_error_windows over a three-stream corpus (a view: channel stride above T), 1, 9 and 17
    windows drawn on the device: the window-table kernel in front of encode_streams_kernel<QUAD, IN planar, REC>, rows + statistics +
    images and statistics alone, without trials and with two.  Per window the crop's ob.encode image, its decode laid out by
    window_oracle.window_expected, the integer sums; a window past its stream: the header with num_samples 0, zero rows and records."""
    import torch
    ch, bits, ms = fmt
    spb = spb_of(ch, bits)
    total, frames = 3 * spb + 7, spb + 19
    lens = [total, spb + 3, 5]
    with restored(engine):
        for dtype in (np.int16, np.float32):
            rows = make_rows(np.random.default_rng(ch + bits), ch, [total] * 3, dtype, seed=50 + bits)
            corpus = planar_tensor(torch, rows, view=True)
            for n_windows in STREAMS:
                g = torch.Generator(device="cuda").manual_seed(1000 * n_windows + 10 * bits + ch)
                windows = torch.stack([torch.randint(0, 3, (n_windows,), generator=g, device="cuda", dtype=torch.int64),
                                       torch.randint(0, total, (n_windows,), generator=g, device="cuda", dtype=torch.int64)], dim=1)
                wins = windows.cpu().numpy().tolist()
                crops = [rows[s][:, f:f + max(0, min(frames, lens[s] - f))] for s, f in wins]
                for trials in (0, 2):
                    param = make_parameter(ch, bits, MBS, 48000, ms, trials)
                    head = ob.encode(np.zeros((1, ch), dtype=np.int16), bits, MBS, 48000, ms, trials)[:31]
                    images, decoded = [], []
                    for c in crops:
                        img = ob.encode(np.ascontiguousarray(q(c).T), bits, MBS, 48000, ms, trials) if c.shape[1] else head[:14] + bytes(4) + head[18:]
                        images.append(img)
                        decoded.append(ob.decode(img)[0] if c.shape[1] else np.zeros((0, ch), dtype=np.int16))
                    exp_stats = np.zeros((n_windows, ch, 4), dtype=np.int64)
                    for w, c in enumerate(crops):
                        if c.shape[1]:
                            exp_stats[w] = expected_stats([c], [decoded[w].T])[0]
                    for out_dtype in (np.int16, np.float32):
                        exp_rows = window_expected(decoded, [(w, 0) for w in range(n_windows)], frames, ch, out_dtype)

                        tdt = torch.float32 if out_dtype == np.float32 else torch.int16

                        def run():
                            # the engine's calls allocate with torch.empty: a block the run before has just freed comes back with
                            # that run's (right) contents, so what a kernel failed to write would not show.  The same runs through a
                            # plan, into buffers filled with a pattern first, are the ones that can tell.
                            y, data, stride, stats = engine.reconstruct_windows(corpus, windows, frames, param, dtype=tdt, return_images=True,
                                                                                return_stats=True, num_samples=lens)
                            alone = engine.codec_error_windows(corpus, windows, frames, param, num_samples=lens)
                            table = np.zeros(3, dtype=STREAM_DESC_DTYPE)
                            table["pcm_offset"], table["num_samples"] = np.arange(3, dtype=np.uint64) * np.uint64(corpus.stride(0)), lens
                            p_y = torch.full((n_windows, ch, frames), 77, dtype=tdt, device="cuda")
                            p_data = torch.full((n_windows, stride), 0xA5, dtype=torch.uint8, device="cuda")
                            p_stats, p_alone = (torch.full((n_windows, ch, 4), -7, dtype=torch.int64, device="cuda") for _ in range(2))
                            plan = engine.window_reconstruct_plan(param, table, corpus.stride(1), corpus.dtype)
                            try:
                                plan.run(corpus, windows, frames, out=p_y, data=p_data, stats=p_stats)
                                plan.run(corpus, windows, frames, out=False, stats=p_alone)
                                torch.cuda.synchronize()
                            finally:
                                plan.close()
                            return [[v.cpu().numpy() for v in (y, data, stats, alone)], [v.cpu().numpy() for v in (p_y, p_data, p_stats, p_alone)]]
                        label = ("window reconstruct", role_id(role), fmt, np.dtype(dtype).name, np.dtype(out_dtype).name, n_windows, trials)
                        off, on = off_and_on(engine, role, run)
                        for res in off + on:
                            assert res[0].dtype == exp_rows.dtype and np.array_equal(res[0], exp_rows), (label, "rows", np.argwhere(res[0] != exp_rows)[:2].tolist())
                            for w, img in enumerate(images):
                                assert bytes(res[1][w, :len(img)]) == img, cp.describe_mismatch("%s window %d %s" % (label, w, wins[w]), res[1][w, :len(img)], img)
                            assert np.array_equal(res[2], exp_stats) and np.array_equal(res[3], exp_stats), (label, "statistics")
                        for res in (off[1], on[1]):  # nothing behind an image is written
                            assert all((res[1][w, len(img):] == 0xA5).all() for w, img in enumerate(images)), (label, "bytes behind an image")
                        same(label, off[1], on[1])


@pytest.mark.parametrize("tile_kbytes", [0, 1])
@by_format
@by_role
def test_host_batches(engine, role, fmt, tile_kbytes):
    """encode_host / decode_host / reconstruct_host whole (tile 0) and in 1 KiB tiles - every tile a launch of its own with its own
    role decision, the encoder state staying on the device between a stream's tiles.  Images, PCM and residual == the oracle; the three
    fp64 statistics at tests/test_gpu_reconstruct.py's bar; role on == role off, doubles included."""
    ch, bits, ms = fmt
    with restored(engine):
        engine.set_tile_kbytes(tile_kbytes)
        for trials in (0, 2):
            param = make_parameter(ch, bits, MBS, 48000, ms, trials)
            pcms, want_img, want_dec = interleaved_case(fmt, trials)[:3]
            for streams in STREAMS:
                def run():
                    images = engine.encode_host(pcms[:streams], param)
                    decoded = engine.decode_host(want_img[:streams])
                    rec, stats = engine.reconstruct_host(pcms[:streams], param, residual=False)
                    gap, stats_g = engine.reconstruct_host(pcms[:streams], param, residual=True)
                    return [images, decoded, rec, gap, [_as_tuple(s) for s in stats], [_as_tuple(s) for s in stats_g]]
                label = ("host batches", role_id(role), fmt, tile_kbytes, trials, streams)
                off, on = off_and_on(engine, role, run)
                for res in (off, on):
                    for s in range(streams):
                        assert res[0][s] == want_img[s], cp.describe_mismatch("%s stream %d" % (label, s), res[0][s], want_img[s])
                        assert np.array_equal(res[1][s], want_dec[s]) and np.array_equal(res[2][s], want_dec[s]), (label, "PCM", s)
                        assert np.array_equal(res[3][s], ob.residual(pcms[s], want_dec[s])), (label, "residual", s)
                        exp = ob.error_stats(pcms[s], want_dec[s])
                        for got in (res[4][s], res[5][s]):
                            np.testing.assert_allclose(got, exp, rtol=STATS_RTOL, atol=0, err_msg=str(label))
                            assert got[2] == exp[2] and ob.stats_line(got) == ob.stats_line(exp), (label, s, got, exp)
                same(label, off, on)


# ---- 2. the ROLE decoders on crafted and ragged input --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_groups():
    """the 1100 golden records grouped by format (a host batch is one format): [(key, [(record, image)])]"""
    groups = {}
    for rec in bf.golden_cases():
        key = (rec["channels"], rec["bits"], rec["ms"], rec["block_size"], rec["spb"])
        groups.setdefault(key, []).append((rec, bf.case_of_record(rec)["image"]))
    return list(groups.items())


_golden_off = {}


def golden_hashes(engine, groups):
    return [bf.pcm_hash(got) for _, members in groups for got in engine.decode_host([img for _, img in members])]


@pytest.mark.parametrize("tile_kbytes", [0, 1])
@pytest.mark.parametrize("mapping", ["auto", "quad"])
@pytest.mark.parametrize("role", [0, 3], ids=role_id)
def test_golden_crafted_images_host_batches(engine, golden_groups, role, mapping, tile_kbytes):
    """All 1100 golden bitstreams (step index up to 4087, the clamp-add scan's corners, and the 300 file headers whose
    samples_per_block and block_size do not belong together) through AADHip_DecodeBatch under a role == the compiled reference's
    hashes, and == the role-off hashes.  One- and two-channel groups take decode_split_kernel<.., ROLE> (SplitLds or SplitScratch).

    Why no header can take a ROLE kernel outside its LDS rows (aad_decode_split.hip.h): the
    plan (plan_decode) and the kernel read the SAME samples_per_block, the file header's.  SplitLds is chosen only while coded =
    samples_per_block - 4 <= kLdsResidualMax, and the rows are lds_row = split_lds_row(coded) = ceil16(coded) + 4 dwords, sixteen of
    them.  locate_block gives blk.n <= samples_per_block whatever block_size says, so a recurrence has at most `coded` coded samples.
    residuals_for_recurrence writes out[k0 + j] for k0 + j < coded only (its wide stores need a full chunk: k0 + 16 <= coded), all
    below lds_row.  predict_for_quad's wide reads are whole chunks [16 k, 16 k + 16) for k < full = coded / 16 and, when coded % 16 !=
    0, one tail load [16 full, 16 full + 16): at most ceil16(coded) <= lds_row - 4.  Row w starts at w * lds_row, w < 16, so every
    access stays inside 16 * lds_row dwords.  samples_per_block <= 4: coded = 0, no write and no read.  A block_size too small for
    the samples only shortens blk.avail; the bytes past it read as zero.  The scratch rows (coded > kLdsResidualMax) are strided by
    ceil16(coded) + 16 with or without a role."""
    want = [rec["decoded_sha256"] for _, members in golden_groups for rec, _ in members]
    names = [(rec["name"], key) for key, members in golden_groups for rec, _ in members]
    assert len(want) == 1100 and sum(1 for _, members in golden_groups for rec, _ in members if rec["header_kind"] == "geometry") == 300
    with restored(engine):
        engine.set_mapping(mapping)
        engine.set_tile_kbytes(tile_kbytes)
        if (mapping, tile_kbytes) not in _golden_off:
            engine.set_simd_role(None)
            _golden_off[(mapping, tile_kbytes)] = golden_hashes(engine, golden_groups)
        off = _golden_off[(mapping, tile_kbytes)]
        engine.set_simd_role(role)
        on = golden_hashes(engine, golden_groups)
        for res, what in ((off, "role off"), (on, role_id(role))):
            bad = [names[i] for i in range(len(want)) if res[i] != want[i]]
            assert not bad, (what, mapping, tile_kbytes, len(bad), bad[:5])
        assert on == off


ROLE_BATCHES = [b for b in BATCHES if b[0] <= 2]
_batch_want = {}
_batch_off = {}


def decode_tables(engine, torch, d_img, hd, tables, out_len):
    outs = []
    for table, with_header in tables:
        plan = engine.decode_plan(hd, table, with_header)
        out = torch.full((out_len,), PCM_CANARY, dtype=torch.int16, device="cuda")
        try:
            plan.run(d_img, out)
            torch.cuda.synchronize()
        finally:
            plan.close()
        assert engine.last_error() == "", engine.last_error()
        outs.append(out.cpu().numpy())
    return outs


@pytest.mark.parametrize("mapping", ["auto", "quad"])
@pytest.mark.parametrize("batch", ROLE_BATCHES, ids=lambda b: "%dch%db%s_mbs%d_x%d_last%d_n%d" % (b[0], b[1], "ms" if b[2] else "", b[3], b[4], b[5], b[6]))
@pytest.mark.parametrize("role", [0, 3], ids=role_id)
def test_crafted_same_format_batches_device_plans(engine, role, batch, mapping):
    """the one- and two-channel same-format batches of tests/test_gpu_bitstream_fuzz.py (crafted headers and bodies, 64 to 2300
    streams: split decoder with LDS rows, with scratch rows, and - more workgroups than CUs - no role at all) as device-resident plans
    under a role, with the file header and as bare blocks: == the oracle, == role off, nothing written outside the streams' runs"""
    import torch
    from aad_amd.engine import parse_header
    channels, bits, ms, mbs, blocks, last, streams = batch
    cases = _same_format_batch("batch-%d-%d-%d-%d-%d-%d" % (channels, bits, ms, mbs, blocks, last), streams, channels, bits, ms, mbs, blocks, last)
    spb, block_size, n, size = cases[0]["spb"], cases[0]["block_size"], cases[0]["num_samples"], len(cases[0]["image"])
    if batch not in _batch_want:
        _batch_want[batch] = np.stack([bf.oracle_decode(c["image"]) for c in cases])
    want = _batch_want[batch]
    pitch_pcm, pitch_img = -(-(n * channels) // 8) * 8, -(-size // 128) * 128
    phase = 64 if bits == 3 else 37
    flat = np.zeros(phase + streams * pitch_img + 256, dtype=np.uint8)
    for i, c in enumerate(cases):
        flat[phase + i * pitch_img:phase + i * pitch_img + size] = np.frombuffer(c["image"], dtype=np.uint8)
    d_img = torch.from_numpy(flat).cuda()
    hd = parse_header(cases[0]["image"][:31])
    whole = np.zeros(streams, dtype=STREAM_DESC_DTYPE)
    whole["pcm_offset"] = np.arange(streams, dtype=np.uint64) * np.uint64(pitch_pcm)
    whole["data_offset"] = phase + np.arange(streams, dtype=np.uint64) * np.uint64(pitch_img)
    whole["data_size"], whole["num_samples"] = size, n
    bare = np.zeros(streams * blocks, dtype=STREAM_DESC_DTYPE)
    for k in range(blocks):
        sel = slice(k, None, blocks)
        bare["pcm_offset"][sel] = whole["pcm_offset"] + np.uint64(k * spb * channels)
        bare["data_offset"][sel] = whole["data_offset"] + np.uint64(31 + k * block_size)
        bare["data_size"][sel] = min(block_size, size - 31 - k * block_size)
        bare["num_samples"][sel] = min(spb, n - k * spb)
    tables = [(whole, True), (bare, False)]
    out_len = streams * pitch_pcm + 64
    with restored(engine):
        engine.set_mapping(mapping)
        if (batch, mapping) not in _batch_off:
            engine.set_simd_role(None)
            _batch_off[(batch, mapping)] = decode_tables(engine, torch, d_img, hd, tables, out_len)
        off = _batch_off[(batch, mapping)]
        engine.set_simd_role(role)
        on = decode_tables(engine, torch, d_img, hd, tables, out_len)
        for res, what in ((off, "role off"), (on, role_id(role))):
            for host, label in zip(res, ("whole", "bare blocks")):
                runs = host[:streams * pitch_pcm].reshape(streams, pitch_pcm)
                got = runs[:, :n * channels].reshape(streams, n, channels)
                bad = np.argwhere((got != want).any(axis=(1, 2)))
                assert bad.size == 0, (what, mapping, label, batch, "stream", int(bad[0][0]), cases[int(bad[0][0])]["header_kind"], cases[int(bad[0][0])]["body_kind"])
                assert (runs[:, n * channels:] == PCM_CANARY).all() and (host[streams * pitch_pcm:] == PCM_CANARY).all(), (what, mapping, label, batch, "wrote outside its rows")
        same(("same-format batch", batch, mapping, role_id(role)), off, on)


CRAFTED = [c for c in DOZEN if c["channels"] <= 2]
LONG_BLOCKS = 20
_crafted = {}


def crafted_case(name):
    """-> (case, pcm, oracle image, oracle decode); "long" = the long 2-bit chain (tone_p6: the weights diverge, header shifts of 8
    and more) cut to its first twenty blocks"""
    if name not in _crafted:
        if name == "long":
            c = dict(LONG_2BIT)
            c["num_samples"] = LONG_BLOCKS * spb_of(1, 2, c["max_block_size"])
        else:
            c = [k for k in CRAFTED if k["name"] == name][0]
        pcm = cp.case_pcm(c)
        image = cp.oracle_encode(c, pcm)
        _crafted[name] = (c, pcm, image, ob.decode(image)[0])
    return _crafted[name]


@pytest.mark.parametrize("name", [c["name"] for c in CRAFTED] + ["long"])
@pytest.mark.parametrize("role", [1, 2], ids=role_id)
def test_crafted_pcm(engine, role, name):
    """tests/crafted_pcm.py's corners (weight shifts up to 13 with wrapping sums, both rails for whole blocks, the step index at rest on
    0 and across its range) through one chain under a role: encode_uniform = Quad with the elected wave (trials: single lanes; dual
    lanes keep QuadDual), decode_uniform = the ROLE split decoder over 6 - 20 recurrences, LDS rows or - 4024 coded samples a block,
    the long 2-bit chain - scratch rows"""
    import torch
    c, pcm, want, decoded = crafted_case(name)
    assert len(CRAFTED) >= 6 and (name != "long" or (c["bits"], c["channels"], len(pcm)) == (2, 1, LONG_BLOCKS * 4028))
    param = make_parameter(c["channels"], c["bits"], c["max_block_size"], 48000, c["ms"], c["trials"])
    d_pcm = torch.from_numpy(pcm[None]).cuda()
    with restored(engine):
        for lanes in (("single", "dual") if c["trials"] else ("dual",)):
            engine.set_mapping("auto", lanes)

            def run():
                d_img, size = engine.encode_uniform(d_pcm, param)
                d_dec, _ = engine.decode_uniform(d_img, size)
                torch.cuda.synchronize()
                return [d_img[0, :size].cpu().numpy(), d_dec[0].cpu().numpy()]
            off, on = off_and_on(engine, role, run)
            for res in (off, on):
                assert bytes(res[0]) == want, cp.describe_mismatch("%s, %s, %s lanes" % (name, role_id(role), lanes), res[0], want)
                assert np.array_equal(res[1], decoded), cp.describe_pcm_mismatch("%s, %s" % (name, role_id(role)), res[1], decoded, want)
            same((name, role_id(role), lanes), off, on)


# (channels, bits, ms, max_block_size): residual rows in LDS - the smallest rows, mid/side, the largest (1976 coded samples) - and in
# the scratch buffer (mono 3-bit at 1024: 2680 coded samples)
RAGGED_GEOMETRIES = [(1, 4, False, 256), (2, 3, True, 256), (2, 2, False, 1024), (1, 3, False, 1024)]


def ragged_streams(tag, channels, bits, ms, mbs, recurrences, turn):
    """crafted streams (bitstream_fuzz.make_case: adversarial headers and bodies) of 1, 2 and 3 blocks whose last block holds 1, 4, 5,
    19 and spb samples, taken in turn (from position `turn` of both cycles on) until the batch has `recurrences` (blocks x channels;
    the last stream is shortened to fit)"""
    blocks_left = recurrences // channels
    assert blocks_left * channels == recurrences
    spb = spb_of(channels, bits, mbs)
    out, i = [], 0
    while blocks_left:
        blocks = min(1 + (i + turn) % 3, blocks_left)
        last = (1, 4, 5, 19, spb)[(i + 2 * turn) % 5]
        out.append(bf.make_case("%s/%d" % (tag, i), channels=channels, bits=bits, max_block_size=mbs, ms=ms, blocks=blocks, last=last))
        blocks_left -= blocks
        i += 1
    return out


@pytest.mark.parametrize("geometry", RAGGED_GEOMETRIES, ids=lambda g: "%dch%db%s_mbs%d" % (g[0], g[1], "ms" if g[2] else "", g[3]))
@by_role
def test_ragged_decode_plans(engine, role, geometry):
    """device-resident decode plans over non-uniform descriptors (find_stream instead of the uniform arithmetic): streams of 1, 2 and 3
    blocks with last blocks of 1, 4, 5, 19 and spb samples, batches of 15, 16 and 17 recurrences (mono; stereo batches have an even
    count: 14, 16 and 18) - one workgroup with an idle row, a full one, two - == the oracle, nothing written outside the runs"""
    import torch
    channels, bits, ms, mbs = geometry
    spb = spb_of(channels, bits, mbs)
    lasts, counts = set(), set()
    with restored(engine):
        for turn, recurrences in enumerate((15, 16, 17) if channels == 1 else (14, 16, 18)):
            cases = ragged_streams("ragged-%d-%d-%d-%d/%d" % (channels, bits, ms, mbs, recurrences), channels, bits, ms, mbs, recurrences, turn)
            lasts |= {c["num_samples"] - (c["num_samples"] - 1) // spb * spb for c in cases}
            counts |= {-(-c["num_samples"] // spb) for c in cases}
            images = [c["image"] for c in cases]
            want = [bf.oracle_decode(b) for b in images]
            label = ("ragged plan", role_id(role), geometry, recurrences)
            off, on = off_and_on(engine, role, lambda: ragged_decode(engine, torch, images))
            for res in (off, on):
                for i, c in enumerate(cases):
                    assert np.array_equal(res[i], want[i]), cp.describe_pcm_mismatch("%s stream %d (%d samples)" % (label, i, c["num_samples"]), res[i], want[i])
            same(label, off, on)
    assert lasts >= {1, 4, 5, 19, spb} and counts == {1, 2, 3}, (lasts, counts)


@pytest.mark.parametrize("geometry", RAGGED_GEOMETRIES, ids=lambda g: "%dch%db%s_mbs%d" % (g[0], g[1], "ms" if g[2] else "", g[3]))
@by_role
def test_truncated_images(engine, role, geometry):
    """data_size ends inside the codes of a block: the bytes that are missing read as zero and the blocks that are not there stay as
    the (zero-filled) buffer was - what the oracle's block walk gives.  data_size ends inside a block header: the plan is refused
    (the reference's INSUFFICIENT_DATA) under a role exactly as without, and the context keeps working."""
    import torch
    from aad_amd import AADApiResult, ApiError
    channels, bits, ms, mbs = geometry
    spb = spb_of(channels, bits, mbs)
    pcms = synth_pcm(9, 2 * spb + 19, channels, seed=70 + bits, kind="noise")
    images = [ob.encode(p, bits, mbs, 48000, ms, 0) for p in pcms]
    block_size = ob.geometry(mbs, channels, bits)[1]
    head = 18 * channels
    # the cut: in the codes of block 0, 1 or 2 - one byte behind the header, mid-block, one byte before the block's end
    # (the third block is the short last one: a byte before the image's end)
    sizes = [min(31 + (i % 3) * block_size + head + (1, (block_size - head) // 2, block_size - head - 1)[i // 3], len(images[i]) - 1)
             for i in range(9)]
    assert all(s > 31 + 2 * block_size + head for s in sizes[2::3])
    want = []
    for img, size in zip(images, sizes):
        w = np.zeros((2 * spb + 19, channels), dtype=np.int16)
        buf = np.frombuffer(img[:size], dtype=np.uint8)
        assert ob.lib().aado_decode_stream(buf.ctypes.data, len(buf), 8, w.ctypes.data, len(w), None) == 0
        want.append(w)
    with restored(engine):
        off, on = off_and_on(engine, role, lambda: ragged_decode(engine, torch, images, sizes, fill=0))
        for res in (off, on):
            for i in range(9):
                assert np.array_equal(res[i], want[i]), cp.describe_pcm_mismatch("truncated %s stream %d at %d" % (role_id(role), i, sizes[i]), res[i], want[i])
        same(("truncated", role_id(role), geometry), off, on)
        engine.set_simd_role(role)
        for inside in (1, head - 1):
            with pytest.raises(ApiError) as e:
                ragged_decode(engine, torch, images, [len(b) for b in images[:8]] + [31 + block_size + inside], fill=0)
            assert e.value.code == AADApiResult.INSUFFICIENT_DATA
        assert all(np.array_equal(g, w) for g, w in zip(ragged_decode(engine, torch, images, sizes, fill=0), want))


# ---- 3. the edge of the role's range -------------------------------------------------------------------------------------------

_edge = {}


def edge_case(ch, streams, trials):
    """`streams` five-sample streams of `ch` channels at 4 bits -> (pcm [streams, 5, ch], images [streams, size], decodes)"""
    key = (ch, streams, trials)
    if key not in _edge:
        pcm = synth_pcm(streams, 5, ch, seed=12 + ch, kind="noise")
        images = [ob.encode(p, 4, MBS, 48000, False, trials) for p in pcm]
        _edge[key] = (pcm, np.stack([np.frombuffer(i, dtype=np.uint8) for i in images]), np.stack([ob.decode(i)[0] for i in images]))
    return _edge[key]


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("role", [0, 3], ids=role_id)
def test_the_edge_of_the_roles_range(engine, role, ch):
    """plan_simd_role gives a role while workgroups <= cus (Device::cus = hipDeviceAttributeMultiprocessorCount, torch's
    multi_processor_count).  Five-sample streams, sixteen recurrences a workgroup: 16 cus recurrences are cus workgroups - the last
    batch with a role - and the next batch (mono: 16 cus + 1 recurrences; stereo: 16 cus + 2, a stream more) is cus + 1 workgroups,
    where the same context silently launches one-wave workgroups again.  Every image and every decoded sample of every stream == the
    oracle.  At 16 cus recurrences also with two trials: dual lanes (QuadDual, no role) and single lanes (Quad with TRIALS, a role)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    at_edge = 16 * cus // ch
    with restored(engine):
        for streams, trials, lanes in ((at_edge, 0, "dual"), (at_edge + 1, 0, "dual"), (at_edge, 2, "dual"), (at_edge, 2, "single")):
            pcm, images, decoded = edge_case(ch, streams, trials)
            param = make_parameter(ch, 4, MBS, 48000, False, trials)
            engine.set_mapping("auto", lanes)
            d_pcm = torch.from_numpy(pcm).cuda()

            def run():
                d_img, size = engine.encode_uniform(d_pcm, param)
                d_dec, _ = engine.decode_uniform(d_img, size)
                torch.cuda.synchronize()
                return [d_img.cpu().numpy()[:, :size], d_dec.cpu().numpy()]
            label = ("edge", role_id(role), ch, streams, trials, lanes)
            off, on = off_and_on(engine, role, run)
            for res in (off, on):
                assert np.array_equal(res[0], images), (label, "images of streams", np.argwhere((res[0] != images).any(axis=1))[:5].ravel().tolist())
                assert np.array_equal(res[1], decoded), (label, "PCM of streams", np.argwhere((res[1] != decoded).any(axis=(1, 2)))[:5].ravel().tolist())
            same(label, off, on)


# ---- 4. a second device ----------------------------------------------------------------------------------------------------------

SECOND_DEVICE_SCRIPT = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch
import oracle_binding as ob
from aad_amd.engine import Engine
from aad_amd.synth import synth_pcm

spb = ob.geometry(1024, 2, 2)[2]
assert spb - 4 == 1976
pcm = synth_pcm(16, spb, 2, seed=21, kind="music")
images = [ob.encode(p, 2, 1024, 48000, False, 0) for p in pcm]
want = np.stack([ob.decode(i)[0] for i in images])
host = np.stack([np.frombuffer(i, dtype=np.uint8) for i in images])
for device in (1, 0):  # the process's FIRST role decode runs on device 1
    engine = Engine(device)
    engine.set_simd_role(2)
    d_dec, _ = engine.decode_uniform(torch.from_numpy(host).to("cuda:%%d" %% device), host.shape[1])
    torch.cuda.synchronize(device)
    assert engine.last_error() == "", (device, engine.last_error())
    assert np.array_equal(d_dec.cpu().numpy(), want), "device %%d: the decode differs from the oracle's" %% device
    engine.close()
print("ok")
'''


def test_role_decoder_on_a_second_device(tmp_path):
    """launch_role raises the ROLE kernels' dynamic-LDS limit once per process.  Stereo 2-bit, max_block_size 1024, sixteen one-block
    streams: 1976 coded samples, rows of 16 x 1988 dwords = 124 KiB, above the 64 KiB a kernel has without asking.  A fresh process
    makes its first role decode on device 1 and another on device 0: both == the oracle, neither reports an error."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: whether the once-per-process limit holds on a second device stays open")
    script = tmp_path / "second_device.py"
    script.write_text(SECOND_DEVICE_SCRIPT % (ROOT_DIR, os.path.join(ROOT_DIR, "tests")))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
