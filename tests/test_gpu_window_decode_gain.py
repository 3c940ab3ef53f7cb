"""Window decode with a per-window gain, written or added into float rows (AADHip_WindowDecodePlanRunGain, include/aad_hip.h;
aad_amd/csrc/aad_decode_window_gain.hip.h).

Bar: every row EQUALS, as bit patterns, the torch expression of the definition on the CPU (tests/window_gain_oracle.py over
tests/window_oracle.py and tests/channel_mix_oracle.py), into a buffer with 64 canary bytes on both sides; for ADD the rows hold
random finite values of the type before the run (-0, subnormals, large magnitudes among them).  The gains hold 1, -1, 0, a tiny
one and the oracle's witnesses - gains and old values on which a fused multiply-add, a float16 pack that skips the float32
rounding, or a gain applied before the 2^-15 give other bits - whose samples are the header samples of a crafted stream.
  1. all variants: same-format plans (bits 2 / 3 / 4 x mono, stereo, mid/side, 3 channels), a mixed plan, channel-mix plans in both
     directions; float32, float16, bfloat16; STORE and ADD;
  2. a NULL table: STORE is AADHip_WindowDecodePlanRun byte for byte, ADD into zeros too;
  3. Engine.mix_windows against the definition's roundings, its gains against snr_gains of the oracle statistics;
  4. errors through the C call;
  5. ADD on float16 past the grid cap;
  6. AADHip_ContextSignalNextRun around a gain run of several kernels."""
import struct

import numpy as np
import pytest

import oracle_binding as ob
import window_gain_oracle as go
from aad_amd.capi import AADApiResult, SAMPLE_BFLOAT16, SAMPLE_FLOAT16, SAMPLE_FLOAT32, SAMPLE_INT16
from aad_amd.engine import parse_header, snr_gains
from channel_mix_oracle import channel_mix_expected
from test_gpu_chip_filling_paths import (MAX_GRID, P, chip, encoded_streams, pack_images, policy, spb_of, window_launch,  # noqa: F401
                                         window_tile)
from test_gpu_window_decode import _pack
from test_gpu_window_decode_half import (_block_size_for, _channel_corpus, _corpus_windows, _mixed_corpus, _plain_windows, _signal)
from test_gpu_window_decode_mixed import _compare, _decode_plan_rows
from window_oracle import window_expected
from window_stats_oracle import channel_mix_stats_expected

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A
GUARD = 32  # int16 elements: 64 bytes in front of and behind the rows
KINDS = {"float32": SAMPLE_FLOAT32, "float16": SAMPLE_FLOAT16, "bfloat16": SAMPLE_BFLOAT16}


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def witness():
    w = go.witnesses()
    assert all(len(v) >= 8 for v in w.values()), {k: len(v) for k, v in w.items()}
    return w


def _craft(image, header, ms):
    """the image with the header samples of its blocks 0 and 1 replaced by the witness samples, in every channel (mid/side: in M,
    with S = 0, so L = R = M)"""
    img = bytearray(image)
    ch, bs = header.num_channels, header.block_size
    for b, samples in enumerate(go.witness_histories()):
        pos = 31 + b * bs
        assert pos + 18 * ch <= len(img), "the witness stream needs the headers of two blocks"
        for c in range(ch):
            for j, v in enumerate(samples if not (ms and c == 1) else (0, 0, 0, 0)):
                struct.pack_into(">h", img, pos + 18 * c + 4 + 4 * (3 - j), v)
    return bytes(img)


def _old_bits(rng, shape, name):
    """random finite values of the type as bit patterns: all magnitudes, with -0, +0, subnormals and the largest finite value"""
    if name == "float32":
        bits = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        bits = np.where((bits & 0x7F800000) == 0x7F800000, bits & 0xBFFFFFFF, bits)  # no infinity, no NaN
        special = np.array([0x80000000, 0, 1, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000], dtype=np.uint32)
    else:
        bits = rng.integers(0, 1 << 16, size=shape, dtype=np.uint64).astype(np.uint16)
        mask, clear = (0x7C00, 0xBFFF) if name == "float16" else (0x7F80, 0xBFFF)
        bits = np.where((bits & mask) == mask, bits & clear, bits).astype(np.uint16)
        special = np.array([0x8000, 0, 1, 0x8001, 0x7BFF if name == "float16" else 0x7F7F, 0x3C00 if name == "float16" else 0x3F80],
                           dtype=np.uint16)
    flat = bits.reshape(-1)
    # moderate magnitudes for most elements, so that sums are not all the old value: three in four within [2^-8, 4)
    if name == "float32":
        mod = (rng.uniform(-4, 4, size=flat.shape) * rng.choice([1.0, 2.0 ** -8], size=flat.shape)).astype(np.float32).view(np.uint32)
    else:
        import torch
        mod = go.bits_of(torch.from_numpy(rng.uniform(-4, 4, size=flat.shape) * rng.choice([1.0, 2.0 ** -8], size=flat.shape)).to(go.torch_dtype(name)))
    keep = rng.random(flat.shape) < 0.25
    flat = np.where(keep, flat, mod)
    flat[rng.choice(flat.size, size=min(flat.size, 4 * len(special)), replace=False)] = np.tile(special, 4)[:min(flat.size, 4 * len(special))]
    return flat.reshape(shape)


def _run_gain(torch, plan, d_img, windows_np, frames, channels, name, gain_np, old_bits=None, null_gain=False):
    """a gain run into `out=` between 64-byte canaries -> the rows' bit patterns; old_bits: an ADD run over them"""
    n = len(windows_np)
    count = n * channels * frames
    width = 2 if name == "float32" else 1  # int16 elements per row element
    big = torch.full((count * width + 2 * GUARD,), CANARY, dtype=torch.int16, device="cuda")
    out = big[GUARD:GUARD + count * width].view(go.torch_dtype(name)).view(n, channels, frames)
    if old_bits is not None:
        out.copy_(go.from_bits(old_bits, name))
    gain = None if null_gain else torch.from_numpy(np.ascontiguousarray(gain_np, dtype=np.float32)).cuda()
    got = plan.run(d_img, torch.from_numpy(windows_np).cuda(), frames, go.torch_dtype(name), out=out, gain=gain, accumulate=old_bits is not None)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = big.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[GUARD + count * width:] == CANARY).all(), "wrote outside its rows"
    rows = host[GUARD:GUARD + count * width]
    return rows.view(np.uint32 if name == "float32" else np.uint16).reshape(n, channels, frames)


def _gains_and_windows(windows, stream, spb, seed):
    """the caller's windows with gains 1, -1, 0, a tiny one and random ones, then the witness windows with theirs ->
    (windows, gains, olds to plant: (window, t, old))"""
    rng = np.random.default_rng(seed)
    gains = rng.uniform(-2.0, 2.0, size=len(windows)).astype(np.float32)
    gains[:6] = [1.0, -1.0, 0.0, 2.0 ** -120, -2.0 ** -136, -0.0]
    gains[-4:] = [-1.0, 2.0 ** -130, 1.0, -3.0]  # the stray and wrapped windows: padding under a negative and a tiny gain
    w_windows, w_gains, olds = go.witness_windows(stream, spb)
    olds = [(len(windows) + i, t, old) for i, t, old in olds]
    return np.concatenate([windows, w_windows]), np.concatenate([gains, w_gains]), olds


def _check_all(torch, plan, d_img, windows, gains, olds, rows32, channels, label, seed):
    """STORE and ADD of every type against the oracle; the old rows of ADD hold the witnesses' old values"""
    frames = rows32.shape[2]
    rng = np.random.default_rng(seed)
    for name in go.DTYPES:
        got = _run_gain(torch, plan, d_img, windows, frames, channels, name, gains)
        _compare(got, go.gain_expected(rows32, gains, name), label + (name, "STORE"), windows)
        old = _old_bits(rng, rows32.shape, name)
        for w, t, value in olds:
            if t < frames:
                old[w, :, t] = go.bits_of(torch.tensor([value], dtype=torch.float32).to(go.torch_dtype(name)))[0]
        got = _run_gain(torch, plan, d_img, windows, frames, channels, name, gains, old_bits=old)
        _compare(got, go.gain_expected(rows32, gains, name, old), label + (name, "ADD"), windows)


def _assert_witnesses_present(rows32, windows, gains, olds, witness, n_plain):
    """the rows of the witness windows hold the witness samples where the witness table says"""
    k = n_plain
    for key in ("double_float16", "double_bfloat16", "order"):
        for g, sample in witness[key]:
            t = go.WITNESS_SAMPLES.index(sample) % 4
            assert gains[k] == g and (rows32[k, :, t] == np.float32(sample) / np.float32(32768.0)).all(), (key, k, sample)
            k += 1
    for (w, t, old), (_, g, sample) in zip(olds, witness["fused"]):
        assert w == k and gains[k] == g and (rows32[k, :, t] == np.float32(sample) / np.float32(32768.0)).all(), ("fused", k)
        k += 1
    assert k == len(windows)


# ---- 1. all variants -------------------------------------------------------------------------------------------------------------
def _plain_corpus(channels, bits, ms):
    """9 streams of 2-4 short blocks (a few 16-sample chunks) with ragged ends, one shorter than a block, one image truncated inside
    its last block, stream 5 with the witness samples in the headers of its blocks 0 and 1 -> (images, header)"""
    mbs = _block_size_for(channels, bits, 70 + 20 * bits)
    seed = 9000 + 100 * channels + 10 * bits + int(ms)
    rng = np.random.default_rng(seed)
    spb = ob.geometry(mbs, channels, bits)[2]
    images = []
    for i in range(9):
        ragged = int(rng.integers(0, spb - 5))
        n = (2 + i % 3) * spb - (spb // 3 if i == 6 else ragged)
        if i == 8:
            n = spb // 2 + 3  # shorter than a block
        amplitude = 3 if i == 0 else (3500, 3900, 700, 12000)[i % 4]
        images.append(ob.encode(_signal(n, channels, amplitude, seed + i), bits, mbs, 48000, ms, 0))
    hd = parse_header(images[0][:31])
    assert 48 <= hd.num_samples_per_block <= 160 and hd.num_samples_per_block == spb
    images[5] = _craft(images[5], hd, ms)
    payload = len(images[6]) - 31
    last = payload - (-(-payload // hd.block_size) - 1) * hd.block_size
    assert last > 18 * channels + 6
    images[6] = images[6][:len(images[6]) - (last - 18 * channels) // 2]
    return images, hd


PLAIN = [(c, b, ms) for c, ms in ((1, False), (2, False), (2, True), (3, False)) for b in (4, 3, 2)]


@pytest.mark.parametrize("geometry", PLAIN, ids=lambda g: "%dch%db%s" % (g[0], g[1], "ms" if g[2] else ""))
def test_same_format_plans(engine, witness, geometry):
    import torch
    channels, bits, ms = geometry
    images, hd = _plain_corpus(channels, bits, ms)
    spb = hd.num_samples_per_block
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    assert lengths[8] < spb and lengths[5] >= 2 * spb
    d_img = torch.from_numpy(flat).cuda()
    decoded = _decode_plan_rows(engine, torch, [hd] * len(images), table, d_img)  # D_s of the definition
    for s, img in enumerate(images):
        if s != 6:
            assert np.array_equal(decoded[s], ob.decode(img)[0]), s
    plan = engine.window_decode_plan(hd, table, True)
    try:
        for frames in ((3 * spb) // 2 | 1, 5):  # odd, about 1.5 blocks: rows at every 2-byte alignment, over a block boundary
            plain = _plain_windows(lengths, spb, frames)
            windows, gains, olds = _gains_and_windows(plain, 5, spb, 100 * bits + channels)
            rows32 = window_expected(decoded, windows, frames, channels, np.float32)
            _assert_witnesses_present(rows32, windows, gains, olds, witness, len(plain))
            _check_all(torch, plan, d_img, windows, gains, olds, rows32, channels, (geometry, frames), 7 + bits)
    finally:
        plan.close()


def _crafted(images, index):
    header = parse_header(images[index][:31])
    images = list(images)
    images[index] = _craft(images[index], header, header.ch_process_method != 0)
    return images, [ob.decode(img)[0] for img in images]


def test_mixed_plan(engine, witness):
    import torch
    images, decoded = _crafted(_mixed_corpus()[0], 0)
    headers = [parse_header(img[:31]) for img in images]
    assert len({(h.bits_per_sample, h.ch_process_method) for h in headers}) == 6
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)
    try:
        for frames in (141, 5):
            plain = _corpus_windows(lengths, spbs, frames)
            windows, gains, olds = _gains_and_windows(plain, 0, spbs[0], 31)
            rows32 = window_expected(decoded, windows, frames, 2, np.float32)
            _assert_witnesses_present(rows32, windows, gains, olds, witness, len(plain))
            _check_all(torch, plan, d_img, windows, gains, olds, rows32, 2, ("mixed", frames), 41)
    finally:
        plan.close()


@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_channel_mix_plans(engine, witness, out_channels):
    """to_mono: the witness stream is stereo with L = R (the down-mix of two equal samples is the sample); to_stereo: it is mono,
    stored into both rows - which hold different old values under ADD"""
    import torch
    index = 1 if out_channels == 1 else 0
    images, decoded = _crafted(_channel_corpus()[0], index)
    headers = [parse_header(img[:31]) for img in images]
    assert headers[index].num_channels == 3 - out_channels
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    try:
        for frames in (141, 5):
            plain = _corpus_windows(lengths, spbs, frames)
            windows, gains, olds = _gains_and_windows(plain, index, spbs[index], 51)
            rows32 = channel_mix_expected(decoded, windows, frames, out_channels, np.float32)
            _assert_witnesses_present(rows32, windows, gains, olds, witness, len(plain))
            if out_channels == 1 and frames > 5:
                floor = channel_mix_expected(decoded, windows, frames, 1, np.int16).astype(np.float32) / np.float32(32768.0)
                assert (rows32 != floor).sum() > 100  # the half step is in front of the gain
            _check_all(torch, plan, d_img, windows, gains, olds, rows32, out_channels, ("channel mix", out_channels, frames), 61)
    finally:
        plan.close()


# ---- 2. a NULL table -----------------------------------------------------------------------------------------------------------------
def _plans(engine):
    """(label, plan, rows per window, images, table, block lengths) for each plan kind"""
    out = []
    images, hd = _plain_corpus(2, 4, True)
    flat, table = _pack(images)
    out.append(("plain", engine.window_decode_plan(hd, table, True), 2, flat, table, [hd.num_samples_per_block] * len(images)))
    images, _ = _mixed_corpus()
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    out.append(("mixed", engine.mixed_window_decode_plan(headers, table, True), 2, flat, table, [h.num_samples_per_block for h in headers]))
    images, _ = _channel_corpus()
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    for oc in (1, 2):
        out.append(("mix%d" % oc, engine.channel_mix_window_decode_plan(headers, table, oc, True), oc, flat, table,
                    [h.num_samples_per_block for h in headers]))
    return out


def test_null_gain_is_the_plain_run(engine):
    import torch
    for label, plan, channels, flat, table, spbs in _plans(engine):
        try:
            d_img = torch.from_numpy(flat).cuda()
            lengths = [int(n) for n in table["num_samples"]]
            frames = 141
            windows = _corpus_windows(lengths, spbs, frames)
            d_win = torch.from_numpy(windows).cuda()
            for name in go.DTYPES:
                plain = go.bits_of(plan.run(d_img, d_win, frames, go.torch_dtype(name)).cpu())
                assert plain.any() and not (plain == (0x80000000 if name == "float32" else 0x8000)).any()  # no plain row holds -0
                store = _run_gain(torch, plan, d_img, windows, frames, channels, name, None, null_gain=True)
                assert store.tobytes() == plain.tobytes(), (label, name, "STORE")
                add = _run_gain(torch, plan, d_img, windows, frames, channels, name, None, old_bits=np.zeros_like(plain), null_gain=True)
                assert add.tobytes() == plain.tobytes(), (label, name, "ADD into zeros")
        finally:
            plan.close()


# ---- 3. the noisy-batch recipe -------------------------------------------------------------------------------------------------------
def test_mix_windows_is_a_store_run_then_an_add_run(engine):
    import torch
    s_images, s_decoded = _channel_corpus()
    n_images, n_decoded = _mixed_corpus()
    s_flat, s_table = _pack(s_images)
    n_flat, n_table = _pack(n_images)
    pitch = lambda images: max(len(i) for i in images)
    s_data = torch.zeros((len(s_images), pitch(s_images)), dtype=torch.uint8)
    for i, img in enumerate(s_images):
        s_data[i, :len(img)] = torch.frombuffer(bytearray(img), dtype=torch.uint8)
    n_data = torch.zeros((len(n_images), pitch(n_images)), dtype=torch.uint8)
    for i, img in enumerate(n_images):
        n_data[i, :len(img)] = torch.frombuffer(bytearray(img), dtype=torch.uint8)
    s_sizes, n_sizes = [len(i) for i in s_images], [len(i) for i in n_images]
    frames = 141
    s_windows = np.array([(s, f) for s in range(len(s_images)) for f in (0, 33, 200)] + [(len(s_images), 0)], dtype=np.int64)
    n_windows = np.array([((3 * k) % len(n_images), 17 * k) for k in range(len(s_windows))], dtype=np.int64)
    n_windows[3] = (len(n_images), 0)  # no noise there: gain 0
    for channels in (1, 2):
        x32 = channel_mix_expected(s_decoded, s_windows, frames, channels, np.float32)
        y32 = channel_mix_expected(n_decoded, n_windows, frames, channels, np.float32)
        s_stats = channel_mix_stats_expected(s_decoded, s_windows, frames, channels)
        n_stats = channel_mix_stats_expected(n_decoded, n_windows, frames, channels)
        want_gains = snr_gains(torch.from_numpy(s_stats), torch.from_numpy(n_stats), 6.0)
        assert (want_gains > 0).sum() >= len(s_windows) - 4 and want_gains[3] == 0 and want_gains[-1] == 0
        for name in ("float32", "float16"):
            rows, gains = engine.mix_windows((s_data.cuda(), s_sizes, torch.from_numpy(s_windows).cuda()),
                                             (n_data.cuda(), n_sizes, torch.from_numpy(n_windows).cuda()), frames, 6.0,
                                             dtype=go.torch_dtype(name), channels=channels)
            assert rows.dtype == go.torch_dtype(name) and rows.shape == (len(s_windows), channels, frames)
            assert torch.equal(gains.cpu(), want_gains), (channels, name)
            first = go.gain_expected(x32, np.ones(len(s_windows), dtype=np.float32), name)
            want = go.gain_expected(y32, want_gains.numpy(), name, first)
            _compare(go.bits_of(rows.cpu()), want, ("mix_windows", channels, name), s_windows)


# ---- 4. errors, through the C call ---------------------------------------------------------------------------------------------------
def test_argument_errors(engine):
    import torch
    lib, bad, ok = engine.lib, AADApiResult.INVALID_ARGUMENT, AADApiResult.OK
    frames = 100
    for label, plan, channels, flat, table, _ in _plans(engine):
        try:
            d_img = torch.from_numpy(flat).cuda()
            win = torch.tensor([[1, 0]], dtype=torch.int64, device="cuda")
            gain = torch.tensor([0.5, 0.25], dtype=torch.float32, device="cuda")
            out = torch.full((2 * channels * frames + 256,), CANARY, dtype=torch.int16, device="cuda")
            run = lambda n, wp, t, kind, op, gp, mode, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRunGain(
                plan.handle, data, n, wp, t, kind, op, gp, mode)
            for kind in KINDS.values():
                for mode in (0, 1):
                    assert run(1, win.data_ptr(), frames, kind, out.data_ptr(), gain.data_ptr() + 1, mode) == bad  # misaligned gain
                    assert run(1, win.data_ptr(), frames, kind, out.data_ptr(), gain.data_ptr() + 2, mode) == bad
                    assert run(1, win.data_ptr(), frames, kind, None, gain.data_ptr(), mode) == bad               # a null out
                    assert run(1, None, frames, kind, out.data_ptr(), gain.data_ptr(), mode) == bad
                    assert run(1, win.data_ptr(), frames, kind, out.data_ptr(), gain.data_ptr(), mode, data=None) == bad
                    assert run(1, win.data_ptr(), 0, kind, out.data_ptr(), gain.data_ptr(), mode) == bad
                    assert run((1 << 63) // channels, win.data_ptr(), 2, kind, out.data_ptr(), gain.data_ptr(), mode) == bad
                    assert run(0, None, frames, kind, None, None, mode, data=None) == ok                          # N = 0: nulls are fine
                    assert run(0, win.data_ptr(), frames, kind, out.data_ptr(), gain.data_ptr(), mode) == ok
                for mode in (2, -1, 1 << 8):                                                                     # no mode
                    assert run(1, win.data_ptr(), frames, kind, out.data_ptr(), gain.data_ptr(), mode) == bad, (label, mode)
            for mode in (0, 1):
                assert run(1, win.data_ptr(), frames, SAMPLE_INT16, out.data_ptr(), gain.data_ptr(), mode) == bad  # int16 rows
                assert run(1, win.data_ptr(), frames, SAMPLE_INT16, out.data_ptr(), None, mode) == bad
                for kind in (2, 3, 6, -1):
                    assert run(1, win.data_ptr(), frames, kind, out.data_ptr(), gain.data_ptr(), mode) == bad
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == CANARY).all()  # no refused run and no N = 0 run wrote
            # a run on an `out` offset by 64 elements, a gain table offset by one float: the canaries on both sides stay
            for kind, width in ((SAMPLE_FLOAT16, 1), (SAMPLE_FLOAT32, 2)):
                out.fill_(CANARY)
                assert run(1, win.data_ptr(), frames, kind, out.data_ptr() + 64 * 2 * width, gain.data_ptr() + 4, 0) == ok
                torch.cuda.synchronize()
                host = out.cpu().numpy()
                lo, hi = 64 * width, 64 * width + channels * frames * width
                assert (host[:lo] == CANARY).all() and (host[hi:] == CANARY).all(), (label, kind)
                assert (host[lo:hi] != CANARY).any()
        finally:
            plan.close()


# ---- 5. past the grid cap ----------------------------------------------------------------------------------------------------------
def test_add_on_float16_past_the_grid_cap(engine, policy, chip):
    """the geometry of tests/test_gpu_chip_filling_paths.py::test_window_decode_past_the_grid_cap: 2^26 + 37 windows of two frames
    over stereo M/S 4-bit streams, 2^28 + 148 lanes under a grid capped at 2^20 workgroups - the last 37 windows are the second trip
    of the grid-stride loop.  An ADD run on float16 rows that hold 0.5, a gain per window."""
    import torch
    ch, bits, frames, tail = 2, 4, 2, 37
    _, spb = spb_of(ch, bits, 64)
    first = 1 << 26
    n = first + tail
    plan = window_launch(policy, chip, n, frames, ch, bits, spb)
    assert plan.ok == 1 and plan.blocks_per_window == 2 and plan.workgroup == 256 and plan.grid == MAX_GRID and plan.lds == 0, plan
    assert plan.lanes == (1 << 28) + 4 * tail and plan.lanes % 64 != 0, plan
    need = n * 16 + n * 4 + n * ch * frames * 2 + (2 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("needs %.1f GiB of free device memory" % (need / 2 ** 30))
    images, decoded, lengths, headers = encoded_streams([(ch, bits, True, 64)] * 3, seed=6100)
    tile = window_tile(lengths, spb, frames, seed=61)
    last = np.array([(0, (1 + i % 3) * spb - 1) for i in range(tail)], dtype=np.int64)
    last[tail // 2] = (len(lengths), 0)
    flat, table = pack_images(images)
    d_img = torch.from_numpy(flat).cuda()
    rng = np.random.default_rng(62)
    tile_gain, last_gain = rng.uniform(-2, 2, size=P).astype(np.float32), rng.uniform(-2, 2, size=tail).astype(np.float32)
    full = first // P
    windows = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    gains = torch.empty((n,), dtype=torch.float32, device="cuda")
    tile_d, tile_g = torch.from_numpy(tile).cuda(), torch.from_numpy(tile_gain).cuda()
    windows[:full * P].view(full, P, 2).copy_(tile_d.unsqueeze(0).expand(full, P, 2))
    windows[full * P:first] = tile_d[:first - full * P]
    windows[first:] = torch.from_numpy(last).cuda()
    gains[:full * P].view(full, P).copy_(tile_g.unsqueeze(0).expand(full, P))
    gains[full * P:first] = tile_g[:first - full * P]
    gains[first:] = torch.from_numpy(last_gain).cuda()
    whole = torch.full((n * ch * frames + 2 * GUARD,), 0.5, dtype=torch.float16, device="cuda")
    whole[:GUARD].view(torch.int16).fill_(CANARY)
    whole[-GUARD:].view(torch.int16).fill_(CANARY)
    y = whole[GUARD:-GUARD].view(n, ch, frames)
    p = engine.window_decode_plan(headers[0], table, True)
    try:
        p.run(d_img, windows, frames, torch.float16, out=y, gain=gains, accumulate=True)
        torch.cuda.synchronize()
    finally:
        p.close()
    edge = whole.view(torch.int16)
    assert bool((edge[:GUARD] == CANARY).all()) and bool((edge[-GUARD:] == CANARY).all()), "wrote outside its rows"
    half = lambda rows32: np.full(rows32.shape, 0x3800, dtype=np.uint16)
    exp = go.gain_expected(window_expected(decoded, tile, frames, ch, np.float32), tile_gain, "float16", half(np.zeros((P, ch, frames))))
    exp_last = go.gain_expected(window_expected(decoded, last, frames, ch, np.float32), last_gain, "float16",
                                half(np.zeros((tail, ch, frames))))
    assert (exp != 0x3800).any() and (exp_last != 0x3800).any()
    got, got_last = go.bits_of(y[:P].cpu()), go.bits_of(y[first:].cpu())
    assert np.array_equal(got, exp), ("first tile", np.argwhere(got != exp)[:3].tolist())
    assert np.array_equal(got_last, exp_last), ("the second trip's windows", np.argwhere(got_last != exp_last)[:3].tolist())
    reps = y[:full * P].view(torch.int16).view(full, P * ch * frames)
    assert bool((reps == reps[0]).all()), "a repetition of the tile differs"
    del windows, gains, whole, y, reps, edge
    torch.cuda.empty_cache()


# ---- 6. signal events ----------------------------------------------------------------------------------------------------------------
def test_signal_next_run_events_around_a_gain_run_of_several_kernels(engine):
    import torch
    from aad_amd.engine import HipEvent
    images, decoded = _mixed_corpus()
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)  # six variants: six kernels
    frames = 141
    windows_np = np.array([(s, (7 * s) % lengths[s]) for s in range(len(images))] * 8, dtype=np.int64)
    gain_np = np.linspace(-2, 2, len(windows_np)).astype(np.float32)
    windows, gain = torch.from_numpy(windows_np).cuda(), torch.from_numpy(gain_np).cuda()
    out = torch.full((len(windows_np), 2, frames), 0.25, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    engine.signal_next(stop, start=start)
    plan.run(d_img, windows, frames, torch.float32, out=out, gain=gain, accumulate=True, ordered=False)
    stop.wait_on(side)
    with torch.cuda.stream(side):
        snapshot = out.clone()
    side.synchronize()
    old = np.full((len(windows_np), 2, frames), np.float32(0.25).view(np.uint32), dtype=np.uint32)
    want = go.gain_expected(window_expected(decoded, windows_np, frames, 2, np.float32), gain_np, "float32", old)
    _compare(go.bits_of(snapshot.cpu()), want, ("events",), windows_np)
    start.synchronize()
    stop.synchronize()
    assert start.elapsed_ms(stop) > 0
    plan.close()
