"""Window decode into float16 and bfloat16 rows (AAD_HIP_SAMPLE_FLOAT16 / AAD_HIP_SAMPLE_BFLOAT16, include/aad_hip.h;
aad_amd/csrc/aad_decode_window.hip.h): the float32 row rounded once to nearest even, from the decode kernels' own stores.

Bar: every row EQUALS, as bit patterns, torch's CPU conversion of the float32 row of the definition
(tests/window_half_oracle.py over tests/window_oracle.py and tests/channel_mix_oracle.py), into a buffer with 64 canary bytes on
both sides.
  1. same-format plans: bits 2 / 3 / 4 x mono, stereo, stereo mid/side, 3 channels; short blocks, ragged streams, one truncated
     image, odd T (rows at every 2-byte alignment), every window edge; the expected rows hold a subnormal (|v| = 1), float16 and
     bfloat16 ties and a rail, asserted before the comparison;
  2. a mixed-format plan;
  3. channel-mix plans in both directions, the down-mix with odd L + R;
  4. statistics: the int16 run's table, rows byte-equal to the run without statistics, a run without rows;
  5. errors, through the C call."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
from aad_amd.capi import (AADApiResult, AADHipPlanarLayout, AADHipPlanarOutput, SAMPLE_BFLOAT16, SAMPLE_FLOAT16, SAMPLE_FLOAT32,
                          SAMPLE_INT16, STREAM_DESC_DTYPE, make_parameter)
from aad_amd.engine import parse_header
from channel_mix_oracle import channel_mix_expected
from test_gpu_window_decode import _pack
from test_gpu_window_decode_channel_mix import _with_history
from test_gpu_window_decode_mixed import _compare, _decode_plan_rows
from window_half_oracle import HALF_DTYPES, half_bits_expected, half_bits_of_float32, torch_dtype
from window_oracle import window_expected

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A
GUARD = 32  # int16 elements: 64 bytes in front of and behind the rows


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _run_bits(torch, plan, d_img, windows_np, frames, channels, dtype, stats=None):
    """a run into `out=` of the dtype between 64-byte canaries -> the [N, C, T] rows as uint16 bit patterns (with stats=True:
    and the table); every element written is the caller's comparison, the canaries untouched is checked here"""
    n = len(windows_np)
    count = n * channels * frames
    big = torch.full((count + 2 * GUARD,), CANARY, dtype=torch.int16, device="cuda")
    out = big[GUARD:GUARD + count].view(dtype).view(n, channels, frames)
    assert out.dtype == dtype and out.data_ptr() == big.data_ptr() + 2 * GUARD
    d_win = torch.from_numpy(windows_np).cuda()
    got = plan.run(d_img, d_win, frames, dtype, out=out, stats=stats)
    table = None
    if stats is not None:
        got, table = got
        table = table.cpu().numpy()
    assert got.data_ptr() == out.data_ptr() and got.dtype == dtype
    host = big.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[GUARD + count:] == CANARY).all(), "wrote outside its rows"
    rows = host[GUARD:GUARD + count].view(np.uint16).reshape(n, channels, frames)
    return rows if stats is None else (rows, table)


def _signal(n, channels, amplitude, seed):
    """a slow sine with a little noise: passes through every value up to its amplitude"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    phase = rng.uniform(0, 6.28, size=(1, channels))
    x = amplitude * np.sin(t * (0.021 + 0.004 * np.arange(channels)[None, :]) + phase) + rng.uniform(-1.5, 1.5, size=(n, channels))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _block_size_for(channels, bits, spb):
    """the largest max_block_size whose blocks hold at most `spb` samples per channel"""
    best = None
    for mbs in range(18 * channels + 1, 18 * channels + 600):
        rc, _, got = ob.geometry(mbs, channels, bits)
        if rc == 0 and 4 < got <= spb:
            best = mbs
    assert best is not None
    return best


RAILS = (32767, -32768, 2049, -257)  # a block's four header samples: both rails, a float16 tie, a bfloat16 tie


def _plain_corpus(channels, bits, ms):
    """8 streams of 2-3 short blocks with ragged ends: a quiet one (amplitude 3), loud ones (a few thousand), one whose block
    headers hold RAILS, one image truncated inside its last block -> (images, header, spb)"""
    mbs = _block_size_for(channels, bits, 100 + 37 * bits)
    seed = 7000 + 100 * channels + 10 * bits + int(ms)
    rng = np.random.default_rng(seed)
    images = []
    for i in range(8):
        spb = ob.geometry(mbs, channels, bits)[2]
        ragged = int(rng.integers(0, spb - 5))
        n = (2 + i % 2) * spb - (spb // 3 if i == 6 else ragged)  # 2 or 3 blocks, the last one ragged (stream 6's: long enough to cut)
        amplitude = 3 if i == 0 else (3500, 3900, 700, 12000)[i % 4]
        images.append(ob.encode(_signal(n, channels, amplitude, seed + i), bits, mbs, 48000, ms, 0))
    hd = parse_header(images[0][:31])
    assert 100 <= hd.num_samples_per_block <= 250
    # stream 5: every block's stored history holds the rails and the ties (mid/side: in M, with S = 0, so L = R = M)
    history = [RAILS] * channels if not ms else [RAILS, (0, 0, 0, 0)]
    images[5] = _with_history({"image": images[5], "channels": channels, "block_size": hd.block_size}, history)
    # stream 6: cut inside the body of its last block
    payload = len(images[6]) - 31
    last = payload - (-(-payload // hd.block_size) - 1) * hd.block_size
    assert last > 18 * channels + 6
    images[6] = images[6][:len(images[6]) - (last - 18 * channels) // 2]
    return images, hd


def _plain_windows(lengths, spb, frames):
    """about 40 windows: per stream a few phases; a start on a block's last frame, an end on a block's first frame; past the end,
    a wrapped first_frame, stray stream indices"""
    rows = []
    for s, n in enumerate(lengths):
        rows += [(s, 0), (s, (n * 3) // 7 + s), (s, max(n - frames, 0)), (s, spb - 1)]
    for k in (1, 2):
        rows += [(1, max(k * spb - frames + 1, 0)), (4, max(k * spb - frames + 1, 0))]  # the last element is the block's first frame
    rows += [(0, lengths[0] - 1), (2, lengths[2]), (3, -1), (3, 1 << 40), (len(lengths), 0), (-1, 5)]
    return np.array(rows, dtype=np.int64)


PLAIN = [(c, b, ms) for c, ms in ((1, False), (2, False), (2, True), (3, False)) for b in (4, 3, 2)]


@pytest.mark.parametrize("geometry", PLAIN, ids=lambda g: "%dch%db%s" % (g[0], g[1], "ms" if g[2] else ""))
def test_plain_plan_rows_are_the_rounded_float32_rows(engine, geometry):
    import torch
    channels, bits, ms = geometry
    images, hd = _plain_corpus(channels, bits, ms)
    spb = hd.num_samples_per_block
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    d_img = torch.from_numpy(flat).cuda()
    decoded = _decode_plan_rows(engine, torch, [hd] * len(images), table, d_img)  # D_s of the definition: AADHip_DecodePlanRun's rows
    for s, img in enumerate(images):
        if s != 6:  # whole images: the CPU oracle's decode
            assert np.array_equal(decoded[s], ob.decode(img)[0]), s
    assert decoded[5][:4, 0].tolist() == list(RAILS) and decoded[5][spb:spb + 4, channels - 1].tolist() == list(RAILS)
    assert np.abs(decoded[0]).max() <= 40 and max(np.abs(d).max() for d in decoded[1:5]) >= 3000
    plan = engine.window_decode_plan(hd, table, True)
    try:
        seen = []
        for frames in (333, 37, 1, 3 * spb + 5):  # odd T: successive rows start at every 2-byte alignment; the last: a zero tail
            windows = _plain_windows(lengths, spb, frames)
            assert 38 <= len(windows) <= 44
            want16 = window_expected(decoded, windows, frames, channels)
            seen.append(np.unique(want16))
            for name in HALF_DTYPES:
                got = _run_bits(torch, plan, d_img, windows, frames, channels, torch_dtype(name))
                _compare(got, half_bits_expected(want16, name), (geometry, frames, name), windows)
            if frames == 3 * spb + 5:
                assert (want16[:, :, -5:] == 0).all() and want16[0].any()  # longer than any stream
        # what the comparison met: a subnormal, a tie of either type, a rail
        mag = np.abs(np.unique(np.concatenate(seen)).astype(np.int32))
        assert (mag == 1).any()
        assert ((mag >= 2048) & (mag < 4096) & (mag % 2 == 1)).any()
        assert ((mag >= 256) & (mag < 512) & (mag % 2 == 1)).any()
        assert (mag >= 32767).any()
    finally:
        plan.close()


# ---- 2. mixed formats --------------------------------------------------------------------------------------------------------------
def _mixed_corpus():
    combos = [(4, 128, False), (3, 256, True), (2, 128, False), (4, 256, True), (3, 128, False), (2, 256, True), (4, 128, False)]
    images = [ob.encode(_signal(300 + 97 * i, 2, (3, 3600, 900, 15000)[i % 4], 8100 + i), bits, mbs, 48000, ms, 0)
              for i, (bits, mbs, ms) in enumerate(combos)]
    return images, [ob.decode(img)[0] for img in images]


def _corpus_windows(lengths, spbs, frames):
    rows = []
    for s, (n, spb) in enumerate(zip(lengths, spbs)):
        rows += [(s, 0), (s, spb - 1), (s, (n * 3) // 7), (s, max(n - frames, 0)), (s, max(spb - frames + 1, 0)), (s, n - 1)]
    rows += [(0, lengths[0]), (1, -1), (len(lengths), 0), (-1, 0)]
    return np.array(rows, dtype=np.int64)


def test_mixed_plan_rows(engine):
    import torch
    images, decoded = _mixed_corpus()
    headers = [parse_header(img[:31]) for img in images]
    assert len({(h.bits_per_sample, h.ch_process_method) for h in headers}) == 6
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.mixed_window_decode_plan(headers, table, True)
    try:
        for frames in (333, 37, 1):
            windows = _corpus_windows(lengths, spbs, frames)
            want16 = window_expected(decoded, windows, frames, 2)
            for name in HALF_DTYPES:
                got = _run_bits(torch, plan, d_img, windows, frames, 2, torch_dtype(name))
                _compare(got, half_bits_expected(want16, name), ("mixed", frames, name), windows)
    finally:
        plan.close()


# ---- 3. channel mix ------------------------------------------------------------------------------------------------------------------
def _channel_corpus():
    combos = [(1, 4, 128, False), (2, 4, 128, False), (2, 3, 256, True), (1, 2, 128, False), (2, 2, 256, False), (1, 3, 256, False),
              (2, 4, 256, True)]
    images = [ob.encode(_signal(280 + 89 * i, ch, (3, 3600, 900, 15000)[i % 4], 8200 + i), bits, mbs, 48000, ms, 0)
              for i, (ch, bits, mbs, ms) in enumerate(combos)]
    return images, [ob.decode(img)[0] for img in images]


@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_channel_mix_plan_rows(engine, out_channels):
    import torch
    images, decoded = _channel_corpus()
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    lengths = [int(n) for n in table["num_samples"]]
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    try:
        for frames in (333, 37, 1):
            windows = _corpus_windows(lengths, spbs, frames)
            want32 = channel_mix_expected(decoded, windows, frames, out_channels, np.float32)
            if out_channels == 1 and frames > 1:
                # the half step is there before the rounding: a float32 row that is not the int16 floor mix / 32768
                want16 = channel_mix_expected(decoded, windows, frames, 1, np.int16)
                assert (want32 != want16.astype(np.float32) / np.float32(32768.0)).sum() > 100
            for name in HALF_DTYPES:
                got = _run_bits(torch, plan, d_img, windows, frames, out_channels, torch_dtype(name))
                _compare(got, half_bits_of_float32(want32, name), ("channel mix", out_channels, frames, name), windows)
                if out_channels == 2:  # a mono stream: two equal rows
                    mono = [w for w, (s, _) in enumerate(windows.tolist()) if 0 <= s < len(headers) and headers[s].num_channels == 1]
                    assert len(mono) >= 18 and got[mono, 0].any() and np.array_equal(got[mono, 0], got[mono, 1])
    finally:
        plan.close()


# ---- 4. statistics ----------------------------------------------------------------------------------------------------------------------
def _plans_for_stats(engine):
    """(label, plan, rows per window, images, stream lengths, block lengths) for each plan kind"""
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


def test_statistics_do_not_depend_on_the_sample_type(engine):
    import torch
    for label, plan, channels, flat, table, spbs in _plans_for_stats(engine):
        try:
            d_img = torch.from_numpy(flat).cuda()
            lengths = [int(n) for n in table["num_samples"]]
            for frames in (333, 37):
                windows = _corpus_windows(lengths, spbs, frames)
                d_win = torch.from_numpy(windows).cuda()
                _, want = plan.run(d_img, d_win, frames, torch.int16, stats=True)
                want = want.cpu().numpy()
                assert want[:, :, 0].any() and (want[:, :, 3] == 0).any()
                for name in HALF_DTYPES:
                    dtype = torch_dtype(name)
                    rows, table_got = _run_bits(torch, plan, d_img, windows, frames, channels, dtype, stats=True)
                    assert np.array_equal(table_got, want), (label, frames, name)
                    assert rows.tobytes() == _run_bits(torch, plan, d_img, windows, frames, channels, dtype).tobytes(), (label, frames, name)
                    alone = plan.run(d_img, d_win, frames, dtype, stats=True, rows=False)
                    assert np.array_equal(alone.cpu().numpy(), want), (label, frames, name, "no rows")
        finally:
            plan.close()


def test_engine_level_calls(engine):
    """Engine.decode_windows and decode_windows_mixed with the two dtypes, with and without channels= and return_stats"""
    import torch
    pcm = torch.from_numpy(np.stack([_signal(900, 2, a, 8300 + i) for i, a in enumerate((3, 3700, 800, 14000))])).cuda()
    d_img, size = engine.encode_uniform(pcm, make_parameter(2, 4, 128))
    d_dec, _ = engine.decode_uniform(d_img, size)
    decoded = list(d_dec.cpu().numpy())
    windows = np.array([(s, f) for s in range(4) for f in (0, 1, 77, 500, 899)] + [(4, 0)], dtype=np.int64)
    d_win = torch.from_numpy(windows).cuda()
    frames = 333
    want16 = window_expected(decoded, windows, frames, 2)
    want_mono = channel_mix_expected(decoded, windows, frames, 1, np.float32)
    for name in HALF_DTYPES:
        dtype = torch_dtype(name)
        bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
        y = engine.decode_windows(d_img, size, d_win, frames, dtype)
        assert y.dtype == dtype and np.array_equal(bits(y), half_bits_expected(want16, name))
        y, stats = engine.decode_windows(d_img, size, d_win, frames, dtype, return_stats=True)
        assert np.array_equal(bits(y), half_bits_expected(want16, name))
        assert torch.equal(stats, engine.decode_windows(d_img, size, d_win, frames, torch.int16, return_stats=True)[1])
        y = engine.decode_windows_mixed(d_img, size, d_win, frames, dtype)
        assert np.array_equal(bits(y), half_bits_expected(want16, name))
        y, stats1 = engine.decode_windows_mixed(d_img, size, d_win, frames, dtype, channels=1, return_stats=True)
        assert y.dtype == dtype and np.array_equal(bits(y), half_bits_of_float32(want_mono, name))
        assert torch.equal(stats1, engine.window_levels(d_img, size, d_win, frames, channels=1))
        # the conversion torch itself would have made from the float32 batch
        assert torch.equal(engine.decode_windows(d_img, size, d_win, frames, torch.float32).to(dtype),
                           engine.decode_windows(d_img, size, d_win, frames, dtype))
    with pytest.raises(ValueError, match="torch.float32, torch.int16, torch.float16 or torch.bfloat16"):
        engine.decode_windows(d_img, size, d_win, frames, torch.float64)
    plan = engine.uniform_window_decode_plan(parse_header(bytes(d_img[0, :31].cpu().numpy())), 4, d_img.shape[1], size)
    try:
        with pytest.raises(ValueError):  # `out` of another dtype than asked for
            plan.run(d_img, d_win, frames, torch.float16, out=torch.zeros((len(windows), 2, frames), dtype=torch.bfloat16, device="cuda"))
    finally:
        plan.close()


# ---- 5. errors, through the C call ------------------------------------------------------------------------------------------------------
def test_argument_errors(engine):
    import torch
    lib, bad, ok = engine.lib, AADApiResult.INVALID_ARGUMENT, AADApiResult.OK
    frames = 100
    for label, plan, channels, flat, table, _ in _plans_for_stats(engine):
        try:
            d_img = torch.from_numpy(flat).cuda()
            win = torch.tensor([[1, 0]], dtype=torch.int64, device="cuda")
            out = torch.full((channels * frames + 64,), CANARY, dtype=torch.int16, device="cuda")
            stats = torch.zeros((channels, 4), dtype=torch.int64, device="cuda")
            run = lambda n, wp, t, kind, op, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRun(plan.handle, data, n, wp, t, kind, op)
            run_stats = lambda n, wp, t, kind, op, sp: lib.AADHip_WindowDecodePlanRunStats(plan.handle, d_img.data_ptr(), n, wp, t, kind, op, sp)
            for kind in (2, 3, 6, -1):  # no sample type
                assert run(1, win.data_ptr(), frames, kind, out.data_ptr()) == bad, (label, kind)
                assert run_stats(1, win.data_ptr(), frames, kind, out.data_ptr(), stats.data_ptr()) == bad, (label, kind)
                assert run_stats(1, win.data_ptr(), frames, kind, None, stats.data_ptr()) == bad, (label, kind)
            for kind in (SAMPLE_FLOAT16, SAMPLE_BFLOAT16):  # as int16
                assert run(1, win.data_ptr(), 0, kind, out.data_ptr()) == bad
                assert run(1, None, frames, kind, out.data_ptr()) == bad
                assert run(1, win.data_ptr(), frames, kind, None) == bad
                assert run(1, win.data_ptr(), frames, kind, out.data_ptr(), data=None) == bad
                assert run_stats(1, win.data_ptr(), frames, kind, out.data_ptr(), None) == bad
                assert run((1 << 63) // channels, win.data_ptr(), 2, kind, out.data_ptr()) == bad  # N * C * T overflows 64 bits
                assert run(0, None, frames, kind, None, data=None) == ok                           # N = 0: nothing is launched
                assert run(0, win.data_ptr(), frames, kind, out.data_ptr()) == ok
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == CANARY).all() and not stats.cpu().numpy().any()  # no refused run and no N = 0 run wrote
            assert run(1, win.data_ptr(), frames, SAMPLE_FLOAT16, out.data_ptr() + 64) == ok
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            assert (host[:32] == CANARY).all() and (host[32 + channels * frames:] == CANARY).all()
            assert (host[32:32 + channels * frames] != CANARY).any()
        finally:
            plan.close()


def test_encode_side_entry_points_still_refuse_the_half_types(engine):
    import torch
    lib, bad = engine.lib, AADApiResult.INVALID_ARGUMENT
    param = make_parameter(2, 4, 256)
    table = np.zeros(2, dtype=STREAM_DESC_DTYPE)
    table["pcm_offset"] = [0, 2000]
    table["data_offset"] = [0, 4096]
    table["data_size"] = 4096
    table["num_samples"] = 1000
    engine.planar_reconstruct_plan(param, table, 1000, torch.int16, torch.float32, 2000, 1000).close()  # the arguments below are good ...
    plan = C.c_void_p()
    for kind in (SAMPLE_FLOAT16, SAMPLE_BFLOAT16):                                                      # ... but for the type
        layout, good = AADHipPlanarLayout(kind, 0, 1000), AADHipPlanarLayout(SAMPLE_INT16, 0, 1000)
        output, good_out = AADHipPlanarOutput(kind, 0, 2000, 1000), AADHipPlanarOutput(SAMPLE_FLOAT32, 0, 2000, 1000)
        assert lib.AADHip_PlanarEncodePlanCreate(engine._ctx, C.byref(param), C.byref(layout), None, 2, table.ctypes.data, C.byref(plan)) == bad
        assert lib.AADHip_PlanarReconstructPlanCreate(engine._ctx, C.byref(param), C.byref(layout), C.byref(good_out), None, 2,
                                                      table.ctypes.data, C.byref(plan)) == bad
        assert lib.AADHip_PlanarReconstructPlanCreate(engine._ctx, C.byref(param), C.byref(good), C.byref(output), None, 2,
                                                      table.ctypes.data, C.byref(plan)) == bad
        assert lib.AADHip_WindowReconstructPlanCreate(engine._ctx, C.byref(param), C.byref(layout), None, 2, table.ctypes.data,
                                                      C.byref(plan)) == bad
        assert not plan.value
    # ... and a window reconstruct run asked for rows of a half type
    corpus = torch.zeros((2, 2, 1000), dtype=torch.int16, device="cuda")
    wplan = engine.window_reconstruct_plan(param, table, 1000, torch.int16)
    try:
        win = torch.tensor([[0, 0], [1, 10]], dtype=torch.int64, device="cuda")
        out = torch.full((2 * 2 * 300,), CANARY, dtype=torch.int16, device="cuda")
        for kind in (SAMPLE_FLOAT16, SAMPLE_BFLOAT16):
            output = AADHipPlanarOutput(kind, 0, 600, 300)
            assert lib.AADHip_WindowReconstructPlanRun(wplan.handle, corpus.data_ptr(), 2, win.data_ptr(), 300, 0, None, C.byref(output),
                                                       out.data_ptr(), None) == bad
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == CANARY).all()
    finally:
        wplan.close()
