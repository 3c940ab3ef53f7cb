"""The device-tensor paths at chip-filling launch geometry, against the CPU oracles (tests/test_gpu_ring.py, test_gpu_tiled.py and
test_gpu_trials_high.py run encode_uniform / decode_uniform there; this module the paths added since).

aad_launch_policy.h launches a run differently once it no longer fits one wave per SIMD (one_wave_per_simd: CUs x 256 lanes; the
dense mono encoders already where their one-wave workgroups stop being resident, dense_encode_workgroup): four-wave workgroups that
share one LDS copy of the tables, per-wave code-staging and ring areas, the byte ring (DenseRing), the occupancy pad of unused dynamic
LDS, and for window decode a grid capped at 2^20 workgroups with a grid-stride loop.  Every case here

  * takes its lane count from the device (the threshold + 1, rounded up to what the case needs) and, before it runs, asks the policy
    header itself - tests/launch_policy_driver.cpp and tests/window_policy_driver.cpp built with g++ - for the plan of its batch on
    this device and asserts kernel, workgroup, grid and dynamic LDS: a case that no longer reaches its regime fails;
  * is a tile of P = 257 distinct rows (or windows) repeated cyclically, the batch length no multiple of P or 64: P is prime and
    above 256, so every lane position of a wave and of a four-wave workgroup sees every row over the repetitions.  The rows are ragged
    (1, 3, 4, 5, spb - 1, spb, spb + 1, 2 spb + 13 ... frames: the lanes of a workgroup have different trip counts and tail units);
    a uniform table (the uni.enabled fast path) runs once per encoder path;
  * compares the FIRST tile on the host with the oracles (oracle_binding.encode / decode, segment_oracle, window_oracle,
    window_stats_oracle, channel_mix_oracle, the integer sums of test_gpu_planar_stats.expected_stats), and then every repetition,
    the partial last one included, with the first tile on the device;
  * keeps images, rows and statistics in pattern-filled buffers (0xA5 bytes, 0x5A5A samples, the NaN 0x7FA5A5A5, a pattern in every
    record) and checks every byte outside the defined ones - but for the bytes inside an image's data_size behind its last byte,
    which the byte ring's whole-sector stores may leave as they like - and that the input is unchanged.

Bar: bit-exact.  Block sizes 64 and 300, streams of one sample to three blocks: a case is a few MB of PCM."""
import collections
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import STREAM_DESC_DTYPE, make_parameter
from aad_amd.engine import parse_header
from channel_mix_oracle import channel_mix_expected
from test_gpu_planar_encode import make_rows, q
from test_gpu_planar_stats import expected_stats
from test_gpu_window_decode import _windows_for
from window_oracle import window_expected
from window_stats_oracle import channel_mix_stats_expected, window_stats_expected

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "aad_amd", "csrc")

P = 257                     # distinct rows (windows) of a batch: prime, above a four-wave workgroup
IMG_CANARY = 0xA5
PCM_CANARY = 0x5A5A
F32_CANARY = 0x7FA5A5A5     # a NaN: compared as bits
REC_PATTERN = -0x0123456789ABCDEF  # what every statistics field holds before a run
GUARD = 256                 # bytes (elements, fields) of pattern in front of and behind every output
MAX_GRID = 1 << 20

Chip = collections.namedtuple("Chip", "cus lds")


# ---- the device, the policy drivers ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chip():
    import torch
    props = torch.cuda.get_device_properties(0)
    arch = str(getattr(props, "gcnArchName", "")).split(":")[0]
    if arch != "gfx950":
        pytest.skip("the launch regimes of this module are gfx950's (163 840 bytes of LDS per CU); this device is %r" % arch)
    return Chip(int(props.multi_processor_count), 163840)


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    """the two policy drivers, built against the header the kernels' launches are planned with"""
    out = tmp_path_factory.mktemp("chip_filling_policy")
    exes = {}
    for name in ("launch_policy_driver", "window_policy_driver"):
        exes[name] = str(out / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", exes[name], os.path.join(HERE, name + ".cpp")],
                       check=True)
    return exes


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [o.split() for o in out]


EncodeLaunch = collections.namedtuple("EncodeLaunch", "kernel trials workgroup grid lds")
WindowLaunch = collections.namedtuple("WindowLaunch", "ok blocks_per_window workgroup grid lds lanes elements")


def encode_launches(policy, chip, batches, rec=False, ring=1):
    """batches: [(bits, channels, streams, trials, block_size, ring_ok)] -> their plans on this device under "auto" (rec: under
    plan_reconstruct_encode; ring: the context's AAD_HIP_ENCODE_RING)"""
    lines = ["%s %d %d 0 0 %d -1 -1 0 %d %d %d %d %d %d" % (("R" if rec else "E", chip.cus, chip.lds, ring) + tuple(int(v) for v in b))
             for b in batches]
    return [EncodeLaunch(o[0], int(o[1]), int(o[2]), int(o[3]), int(o[4])) for o in _ask(policy["launch_policy_driver"], lines)]


def window_launch(policy, chip, windows, frames, channels, bits, spb):
    o = _ask(policy["window_policy_driver"], ["W %d %d -1 %d %d %d %d %d" % (chip.cus, chip.lds, windows, frames, channels, bits, spb)])[0]
    return WindowLaunch(*(int(v) for v in o))


def simd_switch(chip):
    """the first lane count past one wave per SIMD"""
    return chip.cus * 256 + 1


def mono_switch(policy, chip, bits, block_size):
    """the first lane count at which the dense mono encoder leaves one-wave workgroups (dense_encode_workgroup: its LDS lets no more
    of them be resident; 49 153 on the MI355X), found by asking the policy wave by wave"""
    counts = [64 * w + 1 for w in range(chip.cus, 4 * chip.cus + 1)]
    plans = encode_launches(policy, chip, [(bits, 1, n, 0, block_size, 1) for n in counts])
    first = [n for n, p in zip(counts, plans) if p.workgroup == 256][0]
    assert chip.cus * 64 < first <= simd_switch(chip)
    return first


def batch_length(at_least):
    """the batch length of a case: no multiple of P, of 64 or of 256"""
    n = int(at_least)
    while n % P == 0 or n % 64 == 0:
        n += 1
    return n


def assert_encode_plan(label, plan, lanes, kernel, lds):
    """lds: True = the ring and / or the pad is expected, False = none"""
    assert (plan.kernel, plan.workgroup, plan.grid, plan.lds != 0) == (kernel, 256, -(-lanes // 256), lds), (label, lanes, plan)


# ---- tiles and their repetitions -------------------------------------------------------------------------------------------------

def bits_view(t):
    """float32 as int32 (NaN canaries compare as bits), everything else as it is"""
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def bits_of(a):
    """bits_view for numpy arrays"""
    return a.view(np.int32) if a.dtype == np.float32 else a


def repeat_rows(torch, tile, n):
    """tile [P, ...] -> [n, ...]: row i = tile[i % P]"""
    reps = -(-n // tile.shape[0])
    return tile.repeat((reps,) + (1,) * (tile.dim() - 1))[:n].contiguous()


def assert_repetitions(label, t, period=P):
    """every repetition of t's first `period` rows, the partial last one included, equals the first - on the device, in chunks whose
    boolean temporary stays below 1 GiB"""
    import torch
    t = bits_view(t)
    n, first = int(t.shape[0]), t[:period]
    full = n // period
    per = max(1, (1 << 30) // max(1, first.numel()))
    for a in range(1, full, per):
        b = min(full, a + per)
        v = t[a * period:b * period].view((b - a, period) + tuple(t.shape[1:]))
        if not torch.equal(v, first.unsqueeze(0).expand_as(v)):
            bad = (v != first.unsqueeze(0)).flatten(2).any(dim=2).nonzero()[0].tolist()
            raise AssertionError((label, "repetition", a + bad[0], "row", bad[1], "differs from the first tile"))
    rest = n - full * period
    if rest and full:
        last = t[full * period:]
        if not torch.equal(last, first[:rest]):
            bad = (last != first[:rest]).flatten(1).any(dim=1).nonzero()[0].tolist()
            raise AssertionError((label, "the partial last repetition, row", bad[0], "differs from the first tile"))


def guarded(torch, shape, dtype, fill):
    """-> (the whole buffer, the view of `shape` between GUARD elements of pattern); the view starts 64-byte aligned for uint8"""
    count = int(np.prod(shape))
    whole = torch.empty(count + 2 * GUARD, dtype=dtype, device="cuda")
    if dtype == torch.float32:
        whole.view(torch.int32).fill_(F32_CANARY)
    else:
        whole.fill_(fill)
    return whole, whole[GUARD:GUARD + count].view(shape)


def assert_guards(label, whole, fill):
    w = bits_view(whole)
    fill = F32_CANARY if whole.dtype.is_floating_point else fill
    assert bool((w[:GUARD] == fill).all()) and bool((w[-GUARD:] == fill).all()), (label, "wrote outside its buffer")


def spb_of(ch, bits, mbs):
    rc, block_size, spb = ob.geometry(mbs, ch, bits)
    assert rc == 0, (ch, bits, mbs)
    return block_size, spb


def ragged_lengths(spb, count=P):
    base = [1, 3, 4, 5, spb - 1, spb, spb + 1, 2 * spb + 13, 20, spb // 2 + 3, 2, 2 * spb]
    return [base[i % len(base)] for i in range(count)]


_tiles = {}


def planar_tile(ch, bits, ms, mbs, dtype, uniform, trials):
    """P distinct rows of a format as [C, n] arrays of the sample type and per row (oracle image, oracle decode [C, n]); computed
    once.  uniform: every row spb + 5 frames (two blocks, the second one short)."""
    key = (ch, bits, ms, mbs, np.dtype(dtype).name, uniform, trials)
    if key not in _tiles:
        _, spb = spb_of(ch, bits, mbs)
        lens = [spb + 5] * P if uniform else ragged_lengths(spb)
        rows = make_rows(np.random.default_rng(1000 * ch + 10 * bits + mbs), ch, lens, dtype, seed=17 * ch + bits + (5 if uniform else 0))
        want = []
        for r in rows:
            img = ob.encode(np.ascontiguousarray(q(r).T), bits, mbs, 48000, ms, trials)
            want.append((img, np.ascontiguousarray(ob.decode(img)[0].T)))
        _tiles[key] = (rows, want)
    return _tiles[key]


def rows_tensor(torch, rows, n):
    """the tile's rows as a [P, C, T] host array (garbage past every row's end) and repeated as an [n, C, T] cuda tensor"""
    ch, t = rows[0].shape[0], max(r.shape[1] for r in rows)
    host = np.full((len(rows), ch, t), 12345, dtype=np.int16) if rows[0].dtype == np.int16 else np.full((len(rows), ch, t), 9.25, dtype=np.float32)
    for i, r in enumerate(rows):
        host[i, :, :r.shape[1]] = r
    return host, repeat_rows(torch, torch.from_numpy(host).cuda(), n)


def assert_input_unchanged(label, x, host):
    import torch
    assert torch.equal(bits_view(x[:P]), bits_view(torch.from_numpy(host).cuda())), (label, "the input changed")
    assert_repetitions(label + ("input",), x)


def image_table(engine, param, lens_tile, n, x, padded, uniform):
    """-> (table of n streams over x [n, C, T], image pitch, per tile row the encoded size and the data_size): images on 64-byte
    boundaries, at least 64 bytes of pattern between one image's data_size and the next image"""
    sizes = np.array([engine.encoded_size(param, int(v)) for v in lens_tile], dtype=np.uint64)
    assert sizes.min() > 0
    dsize = (sizes + np.uint64(63)) // np.uint64(64) * np.uint64(64) if padded else sizes.copy()
    pitch = (int(dsize.max()) + 63) // 64 * 64 + 64
    reps = -(-n // len(lens_tile))
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    d["pcm_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(x.stride(0))
    d["data_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(pitch)
    d["data_size"] = np.tile(dsize, reps)[:n]
    d["num_samples"] = np.tile(np.asarray(lens_tile, dtype=np.uint64), reps)[:n]
    assert uniform == (len(set(lens_tile)) == 1)
    return d, pitch, sizes, dsize


def check_images(label, torch, whole, images, want, sizes, dsize):
    """images [n, pitch] uint8 inside `whole`: the first tile == the oracle's images with the pattern everywhere else (but for
    [size, data_size) of an image), every repetition == the first tile, the guards untouched"""
    assert_guards(label, whole, IMG_CANARY)
    pitch = int(images.shape[1])
    host = images[:P].cpu().numpy()
    exp = np.full((P, pitch), IMG_CANARY, dtype=np.uint8)
    free = np.zeros((P, pitch), dtype=bool)
    for i, (img, _) in enumerate(want):
        assert len(img) == int(sizes[i]), (label, i)
        exp[i, :len(img)] = np.frombuffer(img, dtype=np.uint8)
        free[i, int(sizes[i]):int(dsize[i])] = True
    bad = np.argwhere((host != exp) & ~free)
    assert bad.size == 0, (label, "images: first bad [row, byte]", bad[0].tolist(), "of", len(bad), "size", int(sizes[bad[0][0]]))
    if free.any():  # what the encoder may leave as it likes is no part of the comparison of the repetitions
        free_d = torch.from_numpy(free).cuda()
        full = int(images.shape[0]) // P
        images[:full * P].view(full, P, pitch).masked_fill_(free_d, IMG_CANARY)
        if int(images.shape[0]) > full * P:
            images[full * P:].masked_fill_(free_d[:int(images.shape[0]) - full * P], IMG_CANARY)
    assert_repetitions(label + ("images",), images)


def check_rows(label, whole, y, want, out_dtype):
    """y [n, C, T] inside `whole`: the first tile == the oracle's decode (float32: / 32768, exact) with the canary past every row's
    end, every repetition == the first tile"""
    assert_guards(label, whole, PCM_CANARY)
    host = bits_view(y[:P]).cpu().numpy()
    if out_dtype == np.float32:
        exp = np.full(host.shape, F32_CANARY, dtype=np.int32)
        for i, (_, dec) in enumerate(want):
            exp[i, :, :dec.shape[1]] = (dec.astype(np.float32) / np.float32(32768.0)).view(np.int32)
    else:
        exp = np.full(host.shape, PCM_CANARY, dtype=np.int16)
        for i, (_, dec) in enumerate(want):
            exp[i, :, :dec.shape[1]] = dec
    bad = np.argwhere(host != exp)
    assert bad.size == 0, (label, "rows: first bad [row, channel, frame]", bad[0].tolist(), "of", len(bad))
    assert_repetitions(label + ("rows",), y)


def check_records(label, whole, table, exp):
    """table [n, C, 4] int64 inside `whole`: the first tile == exp, every repetition == the first tile"""
    assert_guards(label, whole, REC_PATTERN)
    host = table[:len(exp)].cpu().numpy()
    bad = np.argwhere(host != exp)
    assert bad.size == 0, (label, "statistics: first bad [row, channel, field]", bad[0].tolist(), host[tuple(bad[0][:2])].tolist(),
                           exp[tuple(bad[0][:2])].tolist())
    assert_repetitions(label + ("statistics",), table, len(exp))


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def ring_engine(monkeypatch):
    """a context created under AAD_HIP_ENCODE_RING=2: the byte ring in every geometry that can take it"""
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    monkeypatch.setenv("AAD_HIP_ENCODE_RING", "2")
    e = Engine(0)
    yield e
    e.close()


# ---- 1. planar encode ------------------------------------------------------------------------------------------------------------

# (channels, bits, M/S, input type, max_block_size, regime): "resident" = the dense mono encoder's own switch, "simd" = one wave per SIMD
ENCODE_CASES = [
    (1, 4, False, np.float32, 64, "resident"), (1, 3, False, np.float32, 300, "resident"), (1, 2, False, np.float32, 64, "resident"),
    (1, 4, False, np.float32, 300, "simd"), (1, 3, False, np.float32, 64, "simd"), (1, 2, False, np.float32, 64, "simd"),
    (2, 4, True, np.int16, 64, "simd"), (2, 4, False, np.float32, 300, "simd"),
    (2, 3, True, np.int16, 64, "simd"), (2, 3, False, np.float32, 64, "simd"),
    (2, 2, True, np.int16, 300, "simd"), (2, 2, False, np.float32, 64, "simd"),
]
RING_CASES = [c for c in ENCODE_CASES if c[0] == 2 and c[1] != 4]


def case_id(c):
    return "%dch%db%s-%s-mbs%d-%s" % (c[0], c[1], "ms" if c[2] else "", np.dtype(c[3]).name, c[4], c[5])


def case_streams(policy, chip, case):
    ch, bits, _, _, mbs, regime = case
    lanes = simd_switch(chip) if regime == "simd" else mono_switch(policy, chip, bits, spb_of(ch, bits, mbs)[0])
    return batch_length(-(-lanes // ch))


def planar_encode_case(engine, policy, chip, case, ring):
    import torch
    ch, bits, ms, dtype, mbs, regime = case
    block_size, _ = spb_of(ch, bits, mbs)
    n = case_streams(policy, chip, case)
    lanes = n * ch
    tdt = torch.float32 if dtype == np.float32 else torch.int16
    for uniform, trials, padded in ((False, 0, False), (False, 0, True), (False, 2, False), (False, 2, True), (True, 0, False)):
        label = ("planar encode", case_id(case), "ring %d" % ring, "uniform" if uniform else "ragged", "trials %d" % trials,
                 "padded" if padded else "exact", n)
        # with the trial search no ring and no pad is planned; without it the ring for mono, stereo 4-bit and (ring 2) every geometry,
        # the pad - riding on the ring's dynamic LDS or alone - for 4-bit batches from one wave per SIMD on
        want_ring = trials == 0 and (ch == 1 or bits == 4 or ring == 2)
        want_lds = want_ring or (trials == 0 and bits == 4 and lanes >= simd_switch(chip) - 1)
        plan = encode_launches(policy, chip, [(bits, ch, n, trials, block_size, 1)], ring=ring)[0]
        assert_encode_plan(label, plan, lanes, "dense-ring" if want_ring else "dense", want_lds)
        assert plan.trials == (trials != 0)

        rows, want = planar_tile(ch, bits, ms, mbs, dtype, uniform, trials)
        host, x = rows_tensor(torch, rows, n)
        param = make_parameter(ch, bits, mbs, 48000, ms, trials)
        d, pitch, sizes, dsize = image_table(engine, param, [r.shape[1] for r in rows], n, x, padded, uniform)
        whole, images = guarded(torch, (n, pitch), torch.uint8, IMG_CANARY)
        assert images.data_ptr() % 64 == 0
        p = engine.planar_encode_plan(param, d, x.stride(1), tdt)
        try:
            p.run(x, images)
            torch.cuda.synchronize()
        finally:
            p.close()
        assert engine.last_error() == "", engine.last_error()
        check_images(label, torch, whole, images, want, sizes, dsize)
        assert_input_unchanged(label, x, host)


@pytest.mark.parametrize("case", ENCODE_CASES, ids=case_id)
def test_planar_encode(engine, policy, chip, case):
    """encode_streams_kernel<.., IN planar int16 / float32> in four-wave workgroups: DenseRing for mono and stereo 4-bit (with the
    occupancy pad on the ring's dynamic LDS for 4-bit batches from one wave per SIMD on), plain Dense for stereo 3- / 2-bit, and the
    TRIALS dense kernel (no ring, no pad); ragged tables with data_size exact and padded to the sector, one uniform table"""
    planar_encode_case(engine, policy, chip, case, ring=1)


@pytest.mark.parametrize("case", RING_CASES, ids=case_id)
def test_planar_encode_ring_forced(ring_engine, policy, chip, case):
    """AAD_HIP_ENCODE_RING=2: the planar stereo 3- and 2-bit ring instantiations, which "auto" never picks"""
    planar_encode_case(ring_engine, policy, chip, case, ring=2)


# ---- 2. planar reconstruct and its statistics ------------------------------------------------------------------------------------

REC_CASES = [ENCODE_CASES[i] for i in (0, 4, 5, 6, 9, 10)]
REC_KINDS = [("i16", False), ("f32", False), ("i16", True), ("f32", True), (None, True)]  # (rows, statistics)


def reconstruct_run(engine, torch, label, param, d, x, in_dtype, out, with_stats, want, sizes, dsize, rows, seg=None):
    """one run of a planar reconstruct plan into pattern-filled images, rows (out: "i16", "f32" or None) and records, all checked"""
    n, ch, t = (int(v) for v in x.shape)
    pitch = int(d["data_offset"][1]) if n > 1 else 64
    whole_i, images = guarded(torch, (n, pitch), torch.uint8, IMG_CANARY)
    out_dtype = {None: None, "i16": torch.int16, "f32": torch.float32}[out]
    whole_y, y = guarded(torch, (n, ch, t), out_dtype, PCM_CANARY) if out else (None, None)
    whole_s, table = guarded(torch, (n, ch, 4), torch.int64, REC_PATTERN) if with_stats else (None, None)
    p = engine.planar_reconstruct_plan(param, d, x.stride(1), in_dtype, out_dtype or in_dtype, ch * t, t, *(seg or (None, 0)))
    try:
        if with_stats:
            p.run(x, images, y, None, stats=table)
        else:
            p.run(x, images, y, None)
        torch.cuda.synchronize()
    finally:
        p.close()
    assert engine.last_error() == "", engine.last_error()
    check_images(label, torch, whole_i, images, want, sizes, dsize)
    if out:
        check_rows(label, whole_y, y, want, np.float32 if out == "f32" else np.int16)
    if with_stats:
        check_records(label, whole_s, table, expected_stats(rows, [dec for _, dec in want]))


@pytest.mark.parametrize("case", REC_CASES, ids=case_id)
def test_planar_reconstruct(engine, policy, chip, case):
    """encode_streams_kernel<.., IN planar, REC 1..5> in four-wave workgroups (int16 rows, float32 rows, each with statistics,
    statistics only), without trials and with one: images == ob.encode, rows == ob.decode, records == the integer sums, every record
    of a pattern-filled table written.  No reconstruct run is ever planned with the byte ring, AAD_HIP_ENCODE_RING=2 included."""
    import torch
    ch, bits, ms, dtype, mbs, regime = case
    block_size, _ = spb_of(ch, bits, mbs)
    n = case_streams(policy, chip, case)
    lanes = n * ch
    tdt = torch.float32 if dtype == np.float32 else torch.int16
    for trials in (0, 1):
        for ring in (1, 2):
            plan = encode_launches(policy, chip, [(bits, ch, n, trials, block_size, 1)], rec=True, ring=ring)[0]
            assert_encode_plan((case_id(case), trials, ring), plan, lanes, "dense", trials == 0 and bits == 4 and lanes >= simd_switch(chip) - 1)
        for uniform in (False, True):
            if uniform and trials:
                continue
            rows, want = planar_tile(ch, bits, ms, mbs, dtype, uniform, trials)
            host, x = rows_tensor(torch, rows, n)
            param = make_parameter(ch, bits, mbs, 48000, ms, trials)
            d, pitch, sizes, dsize = image_table(engine, param, [r.shape[1] for r in rows], n, x, not uniform, uniform)
            for out, with_stats in (REC_KINDS if not uniform else REC_KINDS[3:4]):
                label = ("planar reconstruct", case_id(case), "uniform" if uniform else "ragged", "trials %d" % trials, out, with_stats, n)
                reconstruct_run(engine, torch, label, param, d, x, tdt, out, with_stats, want, sizes, dsize, rows)
            assert_input_unchanged(("planar reconstruct", case_id(case)), x, host)


# ---- 3. segmented planar encode / reconstruct ------------------------------------------------------------------------------------

SEG = (1, 1)  # segment_blocks, warmup_blocks: a chain per block
SEG_CASES = [(2, 4, True, np.int16, 64, "simd"), (1, 2, False, np.float32, 64, "resident"), (2, 3, False, np.float32, 64, "simd")]
_seg_tiles = {}


def segment_tile(ch, bits, ms, mbs, dtype):
    """P streams of 40 to 46 blocks (last blocks of 1, 5, spb - 1, spb ... frames) -> rows, (segmented image, its decode), chains"""
    key = (ch, bits, ms, mbs, np.dtype(dtype).name)
    if key not in _seg_tiles:
        _, spb = spb_of(ch, bits, mbs)
        lens = [(39 + i % 7) * spb + (1, 5, spb - 1, spb, 20, 4)[i % 6] for i in range(P)]
        rows = make_rows(np.random.default_rng(77 * ch + bits), ch, lens, dtype, seed=3 * ch + bits)
        want = []
        for r in rows:
            img = so.segmented_encode(np.ascontiguousarray(q(r).T), bits, SEG[0], SEG[1], mbs, ms=ms, trials=0)
            want.append((img, np.ascontiguousarray(ob.decode(img)[0].T)))
        chains = [len(so.segments(n, spb, SEG[0], SEG[1])) for n in lens]
        _seg_tiles[key] = (rows, want, chains)
    return _seg_tiles[key]


@pytest.mark.parametrize("case", SEG_CASES, ids=case_id)
def test_segmented(engine, policy, chip, case):
    """segment_blocks = 1, warmup_blocks = 1: the CHAIN count passes the switch (a few hundred streams of 40 - 46 blocks).
    encode_streams_kernel<.., SEG, IN planar> and <.., SEG, REC> (rows + statistics, statistics only: the run clears the table and
    the chains add into it) == tests/segment_oracle.py.  A chain table never takes the byte ring."""
    import torch
    ch, bits, ms, dtype, mbs, regime = case
    block_size, _ = spb_of(ch, bits, mbs)
    rows, want, chains = segment_tile(ch, bits, ms, mbs, dtype)
    lanes_min = simd_switch(chip) if regime == "simd" else mono_switch(policy, chip, bits, block_size)
    per_tile = sum(chains)
    n = (lanes_min // ch // per_tile) * P
    total = (n // P) * per_tile
    while total * ch < lanes_min or n % P == 0 or n % 64 == 0:
        total += chains[n % P]
        n += 1
    for rec in (False, True):
        for ring in (1, 2):
            plan = encode_launches(policy, chip, [(bits, ch, total, 0, block_size, 0)], rec=rec, ring=ring)[0]
            assert_encode_plan((case_id(case), rec, ring, n), plan, total * ch, "dense", bits == 4 and total * ch >= simd_switch(chip) - 1)
    tdt = torch.float32 if dtype == np.float32 else torch.int16
    host, x = rows_tensor(torch, rows, n)
    param = make_parameter(ch, bits, mbs, 48000, ms, 0)
    d, pitch, sizes, dsize = image_table(engine, param, [r.shape[1] for r in rows], n, x, False, False)
    label = ("segmented", case_id(case), n, total)
    whole, images = guarded(torch, (n, pitch), torch.uint8, IMG_CANARY)
    p = engine.planar_encode_plan(param, d, x.stride(1), tdt, SEG[0], SEG[1])
    try:
        p.run(x, images)
        torch.cuda.synchronize()
    finally:
        p.close()
    check_images(label + ("encode",), torch, whole, images, want, sizes, dsize)
    for out, with_stats in (("i16" if dtype == np.float32 else "f32", False), ("i16", True), (None, True)):
        reconstruct_run(engine, torch, label + (out, with_stats), param, d, x, tdt, out, with_stats, want, sizes, dsize, rows, seg=SEG)
    assert_input_unchanged(label, x, host)


# ---- 4. window reconstruct -------------------------------------------------------------------------------------------------------

WINREC_CASES = [(2, 4, True, np.int16, 64, "simd"), (1, 3, False, np.float32, 64, "resident"), (2, 2, False, np.float32, 64, "simd")]
_winrec = {}


def window_reconstruct_tile(ch, bits, ms, mbs, dtype, seg):
    """a corpus of five source streams (3 spb + 7, spb + 3, 5, 0 and 2 spb frames) and P windows of spb + 19 frames on it - whole
    windows, short ones (len_w < T, down to one frame) and, spread so that every 256 consecutive windows hold some, strays (stream
    out of range, first_frame at and past the stream's end, wrapped) - with per window the oracle's image, decode and sums"""
    key = (ch, bits, ms, mbs, np.dtype(dtype).name, seg)
    if key not in _winrec:
        _, spb = spb_of(ch, bits, mbs)
        lens, frames = [3 * spb + 7, spb + 3, 5, 0, 2 * spb], spb + 19
        corpus = make_rows(np.random.default_rng(ch + 10 * bits), ch, [max(lens)] * len(lens), dtype, seed=60 + bits)
        rng = np.random.default_rng(500 + bits + ch)
        wins = []
        for i in range(P):
            s = int(rng.integers(0, len(lens)))
            f = int(rng.integers(0, max(lens[s], 1)))
            if i % 41 == 7:
                s, f = [(len(lens), 0), (-1, 3), (0, lens[0]), (1, -5), (2, 1 << 40), (3, 0), ((1 << 63) - 1, 1)][(i // 41) % 7]
            elif i % 5 == 0:
                s, f = 0, (0, spb, 2 * spb, spb - 1, lens[0] - 1, lens[0] - frames, 5)[(i // 5) % 7]
            wins.append((s, f))
        head = ob.encode(np.zeros((1, ch), dtype=np.int16), bits, mbs, 48000, ms, 0)[:31]
        images, decoded, stats = [], [], np.zeros((P, ch, 4), dtype=np.int64)
        for w, (s, f) in enumerate(wins):
            crop = corpus[s][:, f:f + max(0, min(frames, lens[s] - f))] if 0 <= s < len(lens) and 0 <= f < lens[s] else corpus[0][:, :0]
            if crop.shape[1] == 0:
                images.append(head[:14] + bytes(4) + head[18:])
                decoded.append(np.zeros((0, ch), dtype=np.int16))
                continue
            pcm = np.ascontiguousarray(q(crop).T)
            img = ob.encode(pcm, bits, mbs, 48000, ms, 0) if seg is None else so.segmented_encode(pcm, bits, seg[0], seg[1], mbs, ms=ms, trials=0)
            images.append(img)
            decoded.append(ob.decode(img)[0])
            stats[w] = expected_stats([crop], [decoded[w].T])[0]
        assert sum(1 for dd in decoded if 0 < dd.shape[0] < frames) >= 20 and sum(1 for dd in decoded if dd.shape[0] == 0) >= 7
        _winrec[key] = (corpus, lens, frames, np.array(wins, dtype=np.int64), images, decoded, stats)
    return _winrec[key]


@pytest.mark.parametrize("seg", [None, SEG], ids=["serial", "segmented"])
@pytest.mark.parametrize("case", WINREC_CASES, ids=case_id)
def test_window_reconstruct(engine, policy, chip, case, seg):
    """AADHip_WindowReconstructPlanRun with enough windows that the encoder launch behind window_resolve_kernel passes the switch
    (segmented: two chains per window): rows + images + statistics, and the statistics alone, == the oracle per distinct window"""
    import torch
    ch, bits, ms, dtype, mbs, regime = case
    block_size, spb = spb_of(ch, bits, mbs)
    corpus, lens, frames, wins, want_img, decoded, want_stats = window_reconstruct_tile(ch, bits, ms, mbs, dtype, seg)
    chains = 1 if seg is None else -(-(-(-frames // spb)) // seg[0])
    assert chains == (1 if seg is None else 2)
    lanes_min = simd_switch(chip) if regime == "simd" else mono_switch(policy, chip, bits, block_size)
    n = batch_length(-(-lanes_min // (ch * chains)))
    plan = encode_launches(policy, chip, [(bits, ch, n * chains, 0, block_size, 0)], rec=True)[0]
    assert_encode_plan((case_id(case), seg, n), plan, n * chains * ch, "dense", bits == 4 and n * chains * ch >= simd_switch(chip) - 1)

    tdt = torch.float32 if dtype == np.float32 else torch.int16
    total = max(lens)
    host = np.stack(corpus)
    x = torch.from_numpy(host).cuda()
    table = np.zeros(len(lens), dtype=STREAM_DESC_DTYPE)
    table["pcm_offset"], table["num_samples"] = np.arange(len(lens), dtype=np.uint64) * np.uint64(ch * total), lens
    windows = repeat_rows(torch, torch.from_numpy(wins).cuda(), n)
    param = make_parameter(ch, bits, mbs, 48000, ms, 0)
    pitch = -(-engine.encoded_size(param, frames) // 64) * 64 + 64
    p = engine.window_reconstruct_plan(param, table, total, tdt, *(seg or (None, 0)))
    try:
        for out in ("i16", "f32"):
            label = ("window reconstruct", case_id(case), seg, out, n)
            out_np = np.float32 if out == "f32" else np.int16
            whole_i, images = guarded(torch, (n, pitch), torch.uint8, IMG_CANARY)
            whole_y, y = guarded(torch, (n, ch, frames), torch.float32 if out == "f32" else torch.int16, PCM_CANARY)
            whole_s, stats = guarded(torch, (n, ch, 4), torch.int64, REC_PATTERN)
            whole_a, alone = guarded(torch, (n, ch, 4), torch.int64, REC_PATTERN)
            p.run(x, windows, frames, out=y, data=images, stats=stats)
            p.run(x, windows, frames, out=False, stats=alone)
            torch.cuda.synchronize()
            assert engine.last_error() == "", engine.last_error()
            sizes = np.array([len(i) for i in want_img], dtype=np.uint64)
            check_images(label, torch, whole_i, images, [(i, None) for i in want_img], sizes, sizes)
            assert_guards(label, whole_y, PCM_CANARY)
            exp = window_expected(decoded, [(w, 0) for w in range(P)], frames, ch, out_np)  # every element of a row is defined
            got = y[:P].cpu().numpy()
            bad = np.argwhere(bits_of(got) != bits_of(exp))
            assert bad.size == 0, (label, "rows: first bad [window, channel, frame]", bad[0].tolist(), wins[bad[0][0]].tolist())
            assert_repetitions(label + ("rows",), y)
            check_records(label + ("with rows",), whole_s, stats, want_stats)
            check_records(label + ("alone",), whole_a, alone, want_stats)
    finally:
        p.close()
    assert torch.equal(bits_view(x), bits_view(torch.from_numpy(host).cuda())), "the corpus changed"
    assert torch.equal(windows[:P], torch.from_numpy(wins).cuda())


# ---- 5. window decode ------------------------------------------------------------------------------------------------------------

def encoded_streams(formats, seed):
    """formats: [(channels, bits, M/S, max_block_size)], one stream each, of ragged lengths (three blocks and seven frames, a block
    and three, five frames, two blocks, one frame ...); every fourth stream loses the last seven bytes of its image (a truncated
    image: the oracle decodes what is there) -> images, oracle decodes, the table's lengths, headers"""
    from aad_amd.synth import synth_pcm
    images, decoded, lengths, cut = [], [], [], 0
    for i, (ch, bits, ms, mbs) in enumerate(formats):
        block_size, spb = spb_of(ch, bits, mbs)
        n = (3 * spb + 7, spb + 3, 5, 2 * spb, 1, 2 * spb + 9, spb - 1)[i % 7]
        img = ob.encode(synth_pcm(1, n, ch, seed=seed + 13 * i, kind=("music", "noise")[i % 2])[0], bits, mbs, 48000, ms, 0)
        last = (len(img) - 31) - ((len(img) - 31 - 1) // block_size) * block_size
        if i % 4 == 3 and last > 18 * ch + 7:
            img, cut = img[:-7], cut + 1
        images.append(img)
        decoded.append(ob.decode(img)[0])
        lengths.append(n)
    headers = [parse_header(img[:31]) for img in images]
    assert cut >= (len(formats) >= 4), "no image is truncated"
    assert [h.num_samples for h in headers] == lengths and all(d.shape == (n, h.num_channels) for d, n, h in zip(decoded, lengths, headers))
    return images, decoded, lengths, headers


def pack_images(images):
    """images at odd offsets in one buffer -> (uint8 array, table of whole images)"""
    table = np.zeros(len(images), dtype=STREAM_DESC_DTYPE)
    pos = 37
    for i, img in enumerate(images):
        table["data_offset"][i], table["data_size"][i], table["num_samples"][i] = pos, len(img), parse_header(img[:31]).num_samples
        pos += len(img) + 5 + i % 3
    flat = np.zeros(pos + 64, dtype=np.uint8)
    for i, img in enumerate(images):
        o = int(table["data_offset"][i])
        flat[o:o + len(img)] = np.frombuffer(img, dtype=np.uint8)
    return flat, table


def window_tile(lengths, spb, frames, seed):
    """P windows: tests/test_gpu_window_decode.py's mix (block starts, phase spb - 1, past the end, wrapped, stray) and random ones"""
    mix = _windows_for(lengths, spb, frames)
    assert len(mix) < P
    rng = np.random.default_rng(seed)
    s = rng.integers(0, len(lengths), size=P - len(mix))
    f = np.array([rng.integers(0, max(lengths[int(v)], 1)) for v in s], dtype=np.int64)
    tile = np.concatenate([mix, np.stack([s.astype(np.int64), f], axis=1)])
    return tile[rng.permutation(P)]


def window_decode_runs(engine, torch, label, plan, d_img, tile, n, frames, out_channels, want16, want32, want_stats):
    """the int16 and the float32 run, each without and with STATS (and STATS without rows), n windows = the tile repeated, into
    pattern-filled rows and records: the first tile == the oracle, every repetition == the first tile"""
    windows = repeat_rows(torch, torch.from_numpy(tile).cuda(), n)
    for dtype, want in ((torch.int16, want16), (torch.float32, want32)):
        for stats in (False, True):
            whole_y, y = guarded(torch, (n, out_channels, frames), dtype, PCM_CANARY)
            whole_s, table = guarded(torch, (n, out_channels, 4), torch.int64, REC_PATTERN) if stats else (None, None)
            plan.run(d_img, windows, frames, dtype, out=y, stats=table)
            torch.cuda.synchronize()
            assert engine.last_error() == "", engine.last_error()
            lab = label + (str(dtype), "stats" if stats else "plain", n)
            assert_guards(lab, whole_y, PCM_CANARY)
            got = y[:P].cpu().numpy()
            bad = np.argwhere(bits_of(got) != bits_of(want))
            assert bad.size == 0, (lab, "rows: first bad [window, channel, frame]", bad[0].tolist(), tile[bad[0][0]].tolist(), len(bad))
            assert_repetitions(lab + ("rows",), y)
            if stats:
                check_records(lab, whole_s, table, want_stats)
    whole_s, table = guarded(torch, (n, out_channels, 4), torch.int64, REC_PATTERN)
    plan.run(d_img, windows, frames, torch.int16, stats=table, rows=False)
    torch.cuda.synchronize()
    check_records(label + ("statistics alone", n), whole_s, table, want_stats)
    assert torch.equal(windows[:P], torch.from_numpy(tile).cuda())
    assert_repetitions(label + ("windows",), windows)


def assert_window_plan(label, plan, lds, chip):
    assert plan.ok == 1 and plan.blocks_per_window >= 2 and plan.workgroup == 256 and plan.lanes >= simd_switch(chip), (label, plan)
    assert plan.grid == -(-plan.lanes // 256) < MAX_GRID and (plan.lds != 0) == lds, (label, plan)


SAME_FORMATS = [(1, 4, False), (1, 3, False), (2, 4, True), (2, 3, False), (2, 2, True), (3, 3, False), (8, 4, False)]


@pytest.mark.parametrize("fmt", SAME_FORMATS, ids=lambda f: "%dch%db%s" % (f[0], f[1], "ms" if f[2] else ""))
def test_window_decode_same_format(engine, policy, chip, fmt):
    """decode_window_kernel and its STATS variants in 256-thread workgroups: mono and stereo 3- / 2-bit under the occupancy pad
    (dense_decode_lds_pad), stereo 4-bit and the any-channel kernels (CHF = 0) without - asserted - over seven ragged streams, one of
    them truncated, K = 3 blocks per window"""
    import torch
    ch, bits, ms = fmt
    mbs = 64 if ch <= 3 else 300  # eight channel headers alone are 144 bytes
    _, spb = spb_of(ch, bits, mbs)
    images, decoded, lengths, headers = encoded_streams([(ch, bits, ms, mbs)] * 7, seed=2000 + 10 * ch + bits)
    assert sum(len(img) != engine.encoded_size(make_parameter(ch, bits, mbs, 48000, ms, 0), n) for img, n in zip(images, lengths)) == 1
    frames = spb + 3
    k = -(-(frames - 1) // spb) + 1
    n = batch_length(-(-simd_switch(chip) // (k * ch)))
    plan = window_launch(policy, chip, n, frames, ch, bits, spb)
    label = ("window decode", fmt, n)
    assert_window_plan(label, plan, ch == 1 or (ch == 2 and bits != 4), chip)
    assert plan.blocks_per_window == k == 3 and plan.lanes == n * k * ch
    tile = window_tile(lengths, spb, frames, seed=ch + bits)
    flat, table = pack_images(images)
    d_img = torch.from_numpy(flat).cuda()
    p = engine.window_decode_plan(headers[0], table, True)
    try:
        window_decode_runs(engine, torch, label, p, d_img, tile, n, frames, ch,
                           window_expected(decoded, tile, frames, ch), window_expected(decoded, tile, frames, ch, np.float32),
                           window_stats_expected(decoded, tile, frames, ch, lengths=lengths))
    finally:
        p.close()
    assert torch.equal(d_img, torch.from_numpy(flat).cuda()), "the images changed"


STEREO_VARIANTS = [(2, b, ms) for b in (4, 3, 2) for ms in (False, True)]
MONO_VARIANTS = [(1, b, False) for b in (4, 3, 2)]


def variant_launches(policy, chip, headers, n, frames):
    """-> per (channels, bits, M/S) among the headers the plan of its launch: its bits and the smallest block among its streams"""
    groups = {}
    for h in headers:
        key = (h.num_channels, h.bits_per_sample, int(h.num_channels == 2 and h.ch_process_method == 1))
        groups[key] = min(groups.get(key, 1 << 30), h.num_samples_per_block)
    return {key: window_launch(policy, chip, n, frames, key[0], key[1], spb) for key, spb in groups.items()}


def test_window_decode_mixed_format(engine, policy, chip):
    """a mixed-format plan over all six stereo variants (blocks of 64 and 300 bytes, a truncated image among them): six launches,
    each past the switch - the 3- and 2-bit ones under the pad, the 4-bit ones without"""
    import torch
    formats = [(2, b, ms, mbs) for mbs in (64, 300) for b, ms in ((4, False), (3, True), (2, False), (4, True), (3, False), (2, True))]
    images, decoded, lengths, headers = encoded_streams(formats, seed=3100)
    spbs = [h.num_samples_per_block for h in headers]
    frames = min(spbs) + 3
    n = batch_length(-(-simd_switch(chip) // (2 * 2)))
    launches = variant_launches(policy, chip, headers, n, frames)
    assert sorted(launches) == sorted((c, b, int(ms)) for c, b, ms in STEREO_VARIANTS)
    for key, plan in launches.items():
        assert_window_plan(("mixed", key), plan, key[1] != 4, chip)
    tile = window_tile(lengths, min(spbs), frames, seed=31)
    flat, table = pack_images(images)
    d_img = torch.from_numpy(flat).cuda()
    p = engine.mixed_window_decode_plan(headers, table, True)
    try:
        window_decode_runs(engine, torch, ("mixed window decode",), p, d_img, tile, n, frames, 2,
                           window_expected(decoded, tile, frames, 2), window_expected(decoded, tile, frames, 2, np.float32),
                           window_stats_expected(decoded, tile, frames, 2, lengths=lengths))
    finally:
        p.close()


@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_window_decode_channel_mix(engine, policy, chip, out_channels):
    """a channel-mix plan over all nine variants, to mono (the down-mix through pair_swap) and to stereo (twin stores): nine launches,
    each past the switch"""
    import torch
    formats = [(c, b, ms, mbs) for mbs in (64, 300) for c, b, ms in STEREO_VARIANTS[::2] + MONO_VARIANTS + STEREO_VARIANTS[1::2]]
    images, decoded, lengths, headers = encoded_streams(formats, seed=4100)
    spbs = [h.num_samples_per_block for h in headers]
    frames = min(spbs) + 3
    n = batch_length(-(-simd_switch(chip) // 2))  # a mono launch has K >= 2 lanes per window
    launches = variant_launches(policy, chip, headers, n, frames)
    assert sorted(launches) == sorted((c, b, int(ms)) for c, b, ms in STEREO_VARIANTS + MONO_VARIANTS)
    for key, plan in launches.items():
        assert_window_plan(("channel mix", key), plan, key[0] == 1 or key[1] != 4, chip)
    tile = window_tile(lengths, min(spbs), frames, seed=41 + out_channels)
    flat, table = pack_images(images)
    d_img = torch.from_numpy(flat).cuda()
    p = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    try:
        window_decode_runs(engine, torch, ("channel-mix window decode", out_channels), p, d_img, tile, n, frames, out_channels,
                           channel_mix_expected(decoded, tile, frames, out_channels),
                           channel_mix_expected(decoded, tile, frames, out_channels, np.float32),
                           channel_mix_stats_expected(decoded, tile, frames, out_channels, lengths=lengths))
    finally:
        p.close()


# ---- 6. window decode past the grid cap ------------------------------------------------------------------------------------------

def test_window_decode_past_the_grid_cap(engine, policy, chip):
    """2^26 + 37 windows of two frames over stereo M/S 4-bit streams (K = 2, four lanes a window: 2^28 + 148 lanes): the grid is
    capped at 2^20 workgroups and the last 148 lanes are the SECOND trip of the kernels' grid-stride loop, in a wave that is not
    full.  Those 37 windows are real ones at phase spb - 1 (both blocks of a window decode, the M/S pair exchanges through
    pair_swap) over non-zero samples, and one stray; their rows come to the host and are compared with the oracle.  The same-format
    kernel into int16 rows, its STATS variant (a 4 GiB table), and the channel-mix down-mix kernel."""
    import torch
    ch, bits, frames, tail = 2, 4, 2, 37
    _, spb = spb_of(ch, bits, 64)
    first = 1 << 26
    n = first + tail
    plan = window_launch(policy, chip, n, frames, ch, bits, spb)
    assert plan.ok == 1 and plan.blocks_per_window == 2 and plan.workgroup == 256 and plan.grid == MAX_GRID and plan.lds == 0, plan
    assert plan.lanes == (1 << 28) + 4 * tail and plan.lanes % 64 != 0, plan
    need = n * 16 + n * ch * 32 + 2 * n * ch * frames * 2 + (2 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("needs %.1f GiB of free device memory" % (need / 2 ** 30))
    images, decoded, lengths, headers = encoded_streams([(ch, bits, True, 64)] * 3, seed=6100)
    tile = window_tile(lengths, spb, frames, seed=61)
    last = np.array([(0, (1 + i % 3) * spb - 1) for i in range(tail)], dtype=np.int64)  # phase spb - 1 throughout
    last[tail // 2] = (len(lengths), 0)             # the stray
    want_last = window_expected(decoded, last, frames, ch)
    assert lengths[0] >= 3 * spb + 1 and all((want_last[i] != 0).any(axis=1).all() for i in range(tail) if i != tail // 2)
    flat, table = pack_images(images)
    d_img = torch.from_numpy(flat).cuda()
    tile_d, last_d = torch.from_numpy(tile).cuda(), torch.from_numpy(last).cuda()
    full = first // P
    windows = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    windows[:full * P].view(full, P, 2).copy_(tile_d.unsqueeze(0).expand(full, P, 2))
    windows[full * P:first] = tile_d[:first - full * P]
    windows[first:] = last_d
    try:
        for kind in ("same format", "statistics", "down-mix"):
            out_ch = 1 if kind == "down-mix" else ch
            if kind == "down-mix":
                p = engine.channel_mix_window_decode_plan(headers, table, 1, True)
                exp, exp_last = channel_mix_expected(decoded, tile, frames, 1), channel_mix_expected(decoded, last, frames, 1)
            else:
                p = engine.window_decode_plan(headers[0], table, True)
                exp, exp_last = window_expected(decoded, tile, frames, ch), want_last
            whole_y, y = guarded(torch, (n, out_ch, frames), torch.int16, PCM_CANARY)
            whole_s, stats = guarded(torch, (n, out_ch, 4), torch.int64, REC_PATTERN) if kind == "statistics" else (None, None)
            try:
                p.run(d_img, windows, frames, torch.int16, out=y, stats=stats)
                torch.cuda.synchronize()
            finally:
                p.close()
            assert engine.last_error() == "", engine.last_error()
            label = ("past the grid cap", kind)
            assert_guards(label, whole_y, PCM_CANARY)
            got, got_last = y[:P].cpu().numpy(), y[first:].cpu().numpy()
            assert np.array_equal(got, exp), (label, "first tile", np.argwhere(got != exp)[:3].tolist())
            assert np.array_equal(got_last, exp_last), (label, "the second trip's windows", np.argwhere(got_last != exp_last)[:3].tolist(),
                                                        got_last[:2].tolist())
            assert_repetitions(label + ("rows",), y[:first])
            if stats is not None:
                assert_guards(label, whole_s, REC_PATTERN)
                want_s = window_stats_expected(decoded, tile, frames, ch, lengths=lengths)
                want_s_last = window_stats_expected(decoded, last, frames, ch, lengths=lengths)
                assert np.array_equal(stats[:P].cpu().numpy(), want_s) and np.array_equal(stats[first:].cpu().numpy(), want_s_last), label
                assert_repetitions(label + ("statistics",), stats[:first])
            del whole_y, y, whole_s, stats
            torch.cuda.empty_cache()
        assert torch.equal(windows[:P], tile_d) and torch.equal(windows[first:], last_d)
        assert_repetitions(("past the grid cap", "windows"), windows[:first])
    finally:
        del windows
        torch.cuda.empty_cache()
