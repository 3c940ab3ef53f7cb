"""Window decode statistics on the device (AADHip_WindowDecodePlanRunStats, aad_amd/csrc/aad_decode_window_stats.hip.h): the exact
per-row sum of squares, sum of magnitudes, largest magnitude and frame count of a window decode's int16 rows, from the decode
kernels themselves, with or without the rows, for same-format, mixed-format and channel-mix plans.

Bar: every table EQUALS the numpy restatement of the definition (tests/window_stats_oracle.py) over the CPU oracle's decode - for
int16 runs, float32 runs and runs without rows alike - into a prefilled table with guard records on both sides; the rows are
byte for byte AADHip_WindowDecodePlanRun's, into canary-bordered buffers.
  1. same-format plans of every kernel geometry, file images and bare blocks, every edge of the window table;
  2. the mono / stereo corpus through the channel-mix plan (both output counts) and its stereo and mono halves through the
     mixed-format plan: twin rows, the float32 down-mix's half step, the corners of the sum, variants alternating inside a wave,
     stray windows under either first launch;
  3. 16-sample chunks whose square sum passes 2^32 (DC at the rails);
  4. one lane whose sum of magnitudes over a block passes 2^32 (a 2-bit block of 65535 bytes);
  5. truncated images: the statistics follow the rows, the count does not;
  6. the Python level, with a rejection-sampling round trip;
  7. errors and AADHip_ContextSignalNextRun's events."""

import numpy as np
import pytest

import bitstream_fuzz as bf
import crafted_pcm
import oracle_binding as ob
from aad_amd.capi import AADApiResult, SAMPLE_FLOAT32, SAMPLE_INT16, make_parameter
from aad_amd.engine import level_dbfs, parse_header, rmse
from aad_amd.synth import synth_pcm
from channel_mix_oracle import channel_mix_expected
from test_gpu_window_decode import CANARY, _bare, _pack, _run
from test_gpu_window_decode_channel_mix import LR_HISTORY, MS_HISTORY, _corpus, _variant, _with_history
from test_gpu_window_decode_mixed import _corpus as _mixed_corpus
from test_gpu_window_decode_mixed import _decode_plan_rows, _edge_windows
from window_oracle import window_expected
from window_stats_oracle import channel_mix_stats_expected, stats_of_rows, window_counts, window_stats_expected

pytestmark = pytest.mark.gpu

PATTERN = 0x13579BDF02468ACE  # what every record and guard holds before a run
GUARD = 4                     # records in front of and behind the table


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _run_stats(torch, plan, d_img, windows_np, frames, channels, dtype, rows=True):
    """a statistics run into a prefilled table between guard records and (rows=True) a canary-bordered row buffer as _run's;
    -> (the [N, C, T] rows or None, the int64 [N, C, 4] table), guards and borders checked"""
    n = len(windows_np)
    records = n * channels
    table = torch.full(((records + 2 * GUARD) * 4,), PATTERN, dtype=torch.int64, device="cuda")
    stats = table[GUARD * 4:(GUARD + records) * 4].view(n, channels, 4)
    d_win = torch.from_numpy(windows_np).cuda()
    host_rows = None
    if rows:
        count = records * frames
        big = torch.full((count + 32,), CANARY if dtype == torch.int16 else -7.0, dtype=dtype, device="cuda")
        out = big[16:16 + count].view(n, channels, frames)
        got, st = plan.run(d_img, d_win, frames, dtype, out=out, stats=stats)
        assert got.data_ptr() == out.data_ptr()
        host = big.cpu().numpy()
        border = np.concatenate([host[:16], host[16 + count:]])
        assert (border == (CANARY if dtype == torch.int16 else -7.0)).all(), "wrote outside its rows"
        host_rows = host[16:16 + count].reshape(n, channels, frames)
    else:
        st = plan.run(d_img, d_win, frames, dtype, stats=stats, rows=False)
    assert st.data_ptr() == stats.data_ptr()
    host = table.cpu().numpy()
    assert (host[:GUARD * 4] == PATTERN).all() and (host[(GUARD + records) * 4:] == PATTERN).all(), "wrote outside its records"
    return host_rows, host[GUARD * 4:(GUARD + records) * 4].reshape(n, channels, 4)


def _same(got, want, label, windows):
    assert got.dtype == np.int64 and got.shape == want.shape, label
    if not np.array_equal(got, want):
        w, r, _ = [int(v) for v in np.argwhere(got != want)[0]]
        raise AssertionError((label, "window", w, np.asarray(windows)[w].tolist(), "row", r, got[w, r].tolist(), want[w, r].tolist()))


def _check(torch, plan, d_img, want, windows, frames, channels, label):
    """the int16 run, the float32 run and the run without rows (either sample type) give the one table `want`; the rows are
    AADHip_WindowDecodePlanRun's bytes.  -> (int16 rows, float32 rows)"""
    assert len(windows) <= 512
    out = []
    for dtype in (torch.int16, torch.float32):
        rows, stats = _run_stats(torch, plan, d_img, windows, frames, channels, dtype)
        _same(stats, want, label + (str(dtype),), windows)
        assert rows.tobytes() == _run(torch, plan, d_img, windows, frames, channels, dtype).tobytes(), label + (str(dtype), "rows")
        _, alone = _run_stats(torch, plan, d_img, windows, frames, channels, dtype, rows=False)
        _same(alone, want, label + (str(dtype), "no rows"), windows)
        out.append(rows)
    return out


# ---- 1. same-format plans --------------------------------------------------------------------------------------------------------
GEOMETRIES = [(c, b, False) for c in (1, 2, 3, 8) for b in (4, 3, 2)] + [(2, b, True) for b in (4, 3, 2)]


@pytest.mark.parametrize("with_header", [True, False], ids=["file", "bare"])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dch%db%s" % (g[0], g[1], "ms" if g[2] else ""))
def test_same_format_plans_equal_the_oracle(engine, geometry, with_header):
    import torch
    channels, bits, ms = geometry
    lengths = [2999, 777, 1, 1500]
    images = [ob.encode(synth_pcm(1, n, channels, seed=1300 + 11 * i + channels * 31 + bits)[0], bits, 256, 48000, ms, 0)
              for i, n in enumerate(lengths)]
    decoded = [ob.decode(img)[0] for img in images]
    hd = parse_header(images[0][:31])
    spb = hd.num_samples_per_block
    flat, table = _pack(images)
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.window_decode_plan(hd, table if with_header else _bare(table), with_header)
    try:
        for frames in (1, 16, spb - 1, spb, spb + 2, 2999):
            windows = _edge_windows(lengths, [spb] * len(lengths), frames)
            want = window_stats_expected(decoded, windows, frames, channels)
            assert want[:, :, 3].max() == min(frames, 2999) and (want[:, :, 3] == 0).any() and (want[:, :, 3] == 1).any()
            rows16, rows32 = _check(torch, plan, d_img, want, windows, frames, channels, (geometry, with_header, frames))
            assert np.array_equal(rows16, window_expected(decoded, windows, frames, channels))
            assert np.array_equal(stats_of_rows(rows16, want[:, 0, 3]), want)  # the table is that of the rows the run wrote
            assert np.array_equal(rows32.view(np.uint32), (rows16.astype(np.float32) / np.float32(32768.0)).view(np.uint32))
    finally:
        plan.close()


# ---- 2. mixed-format and channel-mix plans -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """the reference, computed once: images, oracle decodes, lengths, headers, packed bytes, table"""
    images, decoded, lengths = _corpus()
    headers = [parse_header(img[:31]) for img in images]
    flat, table = _pack(images)
    return images, decoded, lengths, headers, flat, table


def _half_steps(rows16, rows32):
    """elements of a float32 row that are not the int16 row / 32768: the down-mix's half steps"""
    return int(np.count_nonzero(rows32 != rows16.astype(np.float32) / np.float32(32768.0)))


@pytest.mark.parametrize("with_header", [True, False], ids=["file", "bare"])
@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_channel_mix_corpus(engine, corpus, out_channels, with_header):
    import torch
    images, decoded, lengths, headers, flat, table = corpus
    assert len(images) == 27 and len({_variant(h) for h in headers}) == 9
    spbs = [h.num_samples_per_block for h in headers]
    spb = min(spbs)
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table if with_header else _bare(table), out_channels, with_header)
    try:
        halves = 0
        for frames in (1, 16, spb - 1, spb, spb + 2, 2999):
            windows = _edge_windows(lengths, spbs, frames)
            want = channel_mix_stats_expected(decoded, windows, frames, out_channels)
            rows16, rows32 = _check(torch, plan, d_img, want, windows, frames, out_channels, ("corpus", out_channels, with_header, frames))
            assert np.array_equal(rows16, channel_mix_expected(decoded, windows, frames, out_channels, np.int16))
            assert np.array_equal(rows32, channel_mix_expected(decoded, windows, frames, out_channels, np.float32))
            halves += _half_steps(rows16, rows32)
            if out_channels == 2:  # twin rows: a mono stream's two records are equal (and not empty)
                mono = [w for w, (s, _) in enumerate(windows.tolist()) if 0 <= s < len(headers) and headers[s].num_channels == 1]
                assert len(mono) >= 9 * 8 and want[mono, 0, 0].any()
                assert np.array_equal(want[mono, 0], want[mono, 1])
        # the float32 down-mix keeps the half step in its rows while its table is the int16 one (_check); nowhere else
        assert (halves > 100) if out_channels == 1 else (halves == 0)
    finally:
        plan.close()


@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
def test_mixed_format_halves_of_the_corpus(engine, corpus, channels):
    import torch
    images, decoded, lengths, headers, _, _ = corpus
    keep = [i for i, h in enumerate(headers) if h.num_channels == channels]
    images, decoded, lengths, headers = ([v[i] for i in keep] for v in (images, decoded, lengths, headers))
    assert len({_variant(h) for h in headers}) == (6 if channels == 2 else 3)
    flat, table = _pack(images)
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    for with_header in (True, False):
        plan = engine.mixed_window_decode_plan(headers, table if with_header else _bare(table), with_header)
        try:
            for frames in (1, 16, min(spbs) - 1, min(spbs), min(spbs) + 2, 2999):
                windows = _edge_windows(lengths, spbs, frames)
                want = window_stats_expected(decoded, windows, frames, channels)
                _check(torch, plan, d_img, want, windows, frames, channels, ("mixed", channels, with_header, frames))
        finally:
            plan.close()


def test_corners_of_the_sum_from_crafted_headers(engine):
    """L + R = -65536, 65534, -3, -1 and a clipping M/S pair in every block's header samples: the down-mix's statistic is that of
    (L + R) >> 1 - 32768, 32767, -2, -1 - under both sample types, while the float32 rows hold the halves"""
    import torch
    images = []
    for bits in (4, 3, 2):
        for ms in (False, True):
            case = bf.make_case("mix-corner-%d-%d" % (bits, ms), channels=2, bits=bits, max_block_size=256, ms=ms, blocks=3,
                                body_kind="random", header_kind="encoderlike")
            images.append(_with_history(case, MS_HISTORY if ms else LR_HISTORY))
    mono = bf.make_case("mix-corner-mono", channels=1, bits=4, max_block_size=256, blocks=2)
    images.append(_with_history(mono, [(-32768, 32767, -1, 1)]))
    headers = [parse_header(img[:31]) for img in images]
    decoded = [bf.oracle_decode(img) for img in images]
    lr = decoded[0].astype(np.int32)
    assert (lr[:4, 0] + lr[:4, 1]).tolist() == [-65536, 65534, -3, -1]
    flat, table = _pack(images)
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    windows = np.array([(s, f) for s in range(len(images)) for f in (0, 1, 2, spbs[s] - 1, spbs[s], spbs[s] + 1)], dtype=np.int64)
    for with_header in (False, True):
        for out_channels in (1, 2):
            plan = engine.channel_mix_window_decode_plan(headers, table if with_header else _bare(table), out_channels, with_header)
            try:
                for frames in (3, 4, 700):
                    want = channel_mix_stats_expected(decoded, windows, frames, out_channels)
                    if out_channels == 1 and frames == 4:
                        # window (0, 0): 32768^2 + 32767^2 + 2^2 + 1^2 - the floor mix, not the halves -32768, 32767, -1.5, -0.5
                        assert want[0, 0].tolist() == [32768 ** 2 + 32767 ** 2 + 5, 32768 + 32767 + 3, 32768, 4]
                    rows16, rows32 = _check(torch, plan, d_img, want, windows, frames, out_channels,
                                            ("corners", with_header, out_channels, frames))
                    if out_channels == 1:
                        assert rows32[0, 0, 2] == np.float32(-1.5 / 32768)
                        assert _half_steps(rows16, rows32) > 0
            finally:
                plan.close()


@pytest.mark.parametrize("out_channels", [1, 2], ids=["to_mono", "to_stereo"])
def test_variants_alternate_window_by_window_inside_a_wave(engine, corpus, out_channels):
    """T = 1: one lane per (window, source channel) - mono, stereo L/R and stereo M/S windows in turn inside a wave, every lane its
    own record (a twin lane two, a down-mixed pair one)"""
    import torch
    images, decoded, lengths, headers, flat, table = corpus
    by_variant = {}
    for s, h in enumerate(headers):
        if lengths[s] > 300:
            by_variant.setdefault(_variant(h), s)
    order = sorted(by_variant, key=lambda v: (v[1], v[2], v[0]))
    cycle = [by_variant[v] for v in order]
    assert len(cycle) == 9
    windows = np.array([(cycle[i % 9], (i * 37) % lengths[cycle[i % 9]]) for i in range(256)], dtype=np.int64)
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    try:
        want = channel_mix_stats_expected(decoded, windows, 1, out_channels)
        assert (want[:, :, 3] == 1).all() and (want[:, :, 0] == want[:, :, 2] ** 2).all()
        _check(torch, plan, d_img, want, windows, 1, out_channels, ("wave", out_channels))
    finally:
        plan.close()


@pytest.mark.parametrize("first", ["stereo_source_first", "mono_source_first"])
def test_stray_windows_under_either_first_launch(engine, corpus, first):
    """no lane adds into the record of a window whose stream is out of range: its zeros are the clear's, under a stereo-source
    first launch and under a mono-source one, with other windows around it and alone"""
    import torch
    images, decoded, lengths, headers, _, _ = corpus
    keep = [i for i, h in enumerate(headers) if first == "stereo_source_first" or h.num_channels == 1]
    images, decoded, lengths, headers = ([v[i] for i in keep] for v in (images, decoded, lengths, headers))
    assert any(h.num_channels == 2 for h in headers) == (first == "stereo_source_first")
    flat, table = _pack(images)
    spbs = [h.num_samples_per_block for h in headers]
    d_img = torch.from_numpy(flat).cuda()
    for out_channels in (2, 1):
        plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
        try:
            for frames in (1, min(spbs) + 2, 2999):
                windows = _edge_windows(lengths, spbs, frames)
                stray = [w for w, (s, _) in enumerate(windows.tolist()) if s % (1 << 64) >= len(images)]
                assert len(stray) >= 4
                want = channel_mix_stats_expected(decoded, windows, frames, out_channels)
                assert not want[stray].any()  # all-zero records, count = 0
                _check(torch, plan, d_img, want, windows, frames, out_channels, ("strays", first, out_channels, frames))
                _check(torch, plan, d_img, want[stray], windows[stray], frames, out_channels, ("strays alone", first, out_channels, frames))
        finally:
            plan.close()


# ---- 3. the chunk accumulator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["dc_lo", "dc_hi"])
def test_chunks_whose_square_sum_passes_32_bits(engine, family):
    """DC at a rail, 4-bit, block size 1024: sixteen samples of -32768 are 2^34 in sum_sq - a 32-bit chunk accumulator wraps"""
    import torch
    img = ob.encode(crafted_pcm.generate(family, 3000, 1), 4, 1024, 48000, False, 0)
    decoded = [ob.decode(img)[0]]
    hd = parse_header(img[:31])
    spb = hd.num_samples_per_block
    d = decoded[0][:, 0].astype(np.int64)
    # the first block's 16-sample chunks (behind the four header samples), on the CPU: most pass 2^32
    body = d[4:spb]
    chunks = (body[:len(body) // 16 * 16].reshape(-1, 16) ** 2).sum(axis=1)
    assert (chunks >= 1 << 32).sum() >= len(chunks) // 2 and chunks.max() < 1 << 35
    assert np.abs(d).max() == (32768 if family == "dc_lo" else 32767)
    if family == "dc_lo":
        assert (d == -32768).sum() > 1000
    flat, table = _pack([img])
    d_img = torch.from_numpy(flat).cuda()
    windows = np.array([(0, 0), (0, 4), (0, 5), (0, 20), (0, spb - 1), (0, spb), (0, spb + 3), (0, 2990), (0, 2999), (0, 3000), (1, 0)],
                       dtype=np.int64)
    same = engine.window_decode_plan(hd, table, True)
    mix = engine.channel_mix_window_decode_plan([hd], table, 2, True)  # a twin lane adds the same sums twice
    try:
        for frames in (16, 17, spb, 3000):
            want = window_stats_expected(decoded, windows, frames, 1)
            assert want[0, 0, 0] >= 1 << 32 and want[:, 0, 2].max() == np.abs(d).max()
            if frames == 3000:
                assert want[0, 0, 0] > 1 << 40
            _check(torch, same, d_img, want, windows, frames, 1, (family, "same", frames))
            _check(torch, mix, d_img, np.repeat(want, 2, axis=1), windows, frames, 2, (family, "twin", frames))
    finally:
        same.close()
        mix.close()


# ---- 4. the per-lane accumulator ---------------------------------------------------------------------------------------------------
def test_one_lanes_sum_of_magnitudes_passes_32_bits(engine):
    """mono 2-bit at block size 65535: 262 072 frames per block, one lane decodes them all, and at the lower rail their magnitudes
    sum past 2^32"""
    import torch
    img = ob.encode(crafted_pcm.generate("dc_lo", 270000, 1), 2, 65535, 48000, False, 0)
    decoded = [ob.decode(img)[0]]
    hd = parse_header(img[:31])
    spb = hd.num_samples_per_block
    assert (hd.block_size, spb) == (65535, 262072)
    first_block = int(np.abs(decoded[0][:spb, 0].astype(np.int64)).sum())
    assert first_block > 1 << 32  # one block's - one lane's - share
    flat, table = _pack([img])
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.window_decode_plan(hd, table, True)
    try:
        for window, frames in (((0, 0), 262072), ((0, 5), 264000)):
            windows = np.array([window], dtype=np.int64)
            want = window_stats_expected(decoded, windows, frames, 1)
            assert want[0, 0, 1] > 1 << 32 and want[0, 0, 3] == frames and want[0, 0, 0] > 1 << 47
            _check(torch, plan, d_img, want, windows, frames, 1, ("long block", window, frames))
    finally:
        plan.close()


# ---- 5. truncated images -------------------------------------------------------------------------------------------------------------
def test_truncated_images_change_the_sums_and_not_the_count(engine):
    """the mixed test's cuts: the statistics are those of AADHip_DecodePlanRun's rows of the same bytes, count is the table's"""
    import torch
    images, _, lengths = _mixed_corpus(2)
    headers = [parse_header(img[:31]) for img in images]
    cut = []
    for i, (img, h) in enumerate(zip(images, headers)):
        payload, bs = len(img) - 31, h.block_size
        blocks = -(-payload // bs)
        if i % 4 == 0:
            keep = len(img) - 7 if payload - (blocks - 1) * bs > 36 + 7 else len(img)
        elif i % 4 == 1 and blocks > 1:
            keep = 31 + (blocks // 2) * bs + 36 + (bs - 36) // 3  # inside an earlier block
        elif i % 4 == 2:
            keep = 31 + (blocks - 1) * bs + 36                     # the last block: its channel headers alone
        else:
            keep = len(img)
        cut.append(img[:keep])
    assert sum(len(a) != len(b) for a, b in zip(cut, images)) >= 12
    spbs = [h.num_samples_per_block for h in headers]
    tables = {}
    for name, imgs in (("whole", images), ("cut", cut)):
        flat, table = _pack(imgs)
        assert [int(n) for n in table["num_samples"]] == lengths
        d_img = torch.from_numpy(flat).cuda()
        decoded = _decode_plan_rows(engine, torch, headers, table, d_img)  # AADHip_DecodePlanRun, one plan per format
        plan = engine.mixed_window_decode_plan(headers, table, True)
        try:
            for key, windows, frames in (("streams", np.array([(s, 0) for s in range(len(imgs))], dtype=np.int64), 3000),
                                         ("edges", _edge_windows(lengths, spbs, 301), 301)):
                want = window_stats_expected(decoded, windows, frames, 2, lengths=lengths)
                assert np.array_equal(want[:, 0, 3], window_counts(lengths, windows, frames))
                _check(torch, plan, d_img, want, windows, frames, 2, ("truncated", name, key))
                tables[name, key] = want
        finally:
            plan.close()
    for key in ("streams", "edges"):
        a, b = tables["whole", key], tables["cut", key]
        assert np.array_equal(a[:, :, 3], b[:, :, 3])       # the count is unchanged by the cut ...
        assert (a[:, :, 0] != b[:, :, 0]).sum() >= 8        # ... the sums are not


# ---- 6. Python level -------------------------------------------------------------------------------------------------------------------
def test_python_level_and_rejection_sampling(engine):
    import torch
    n, length, frames = 8, 2500, 700
    pcm = synth_pcm(n, length, 2, seed=61)
    pcm[2] = 0
    pcm[5] = 0  # two silent streams
    x = torch.from_numpy(pcm).cuda()
    d_img, size = engine.encode_uniform(x, make_parameter(2, 4, 256))
    d_dec, _ = engine.decode_uniform(d_img, size)
    decoded = list(d_dec.cpu().numpy())
    assert not decoded[2].any() and not decoded[5].any() and all(decoded[s].any() for s in (0, 1, 3, 4, 6, 7))
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    windows = torch.stack([torch.randint(0, n, (256,), device="cuda", generator=g),
                           torch.randint(0, length - frames // 2, (256,), device="cuda", generator=g)], dim=1)
    host = windows.cpu().numpy()
    assert {2, 5} <= set(host[:, 0].tolist())
    # decode_windows(..., return_stats=True)
    rows, stats = engine.decode_windows(d_img, size, windows, frames, torch.int16, return_stats=True)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (256, 2, 4) and stats.is_cuda
    want = window_stats_expected(decoded, host, frames, 2)
    _same(stats.cpu().numpy(), want, ("decode_windows",), host)
    assert np.array_equal(rows.cpu().numpy(), window_expected(decoded, host, frames, 2))
    assert torch.equal(rows, engine.decode_windows(d_img, size, windows, frames, torch.int16))  # without the keyword: as before
    # decode_windows_mixed(..., channels=1, return_stats=True)
    rows1, stats1 = engine.decode_windows_mixed(d_img, size, windows, frames, channels=1, return_stats=True)
    assert rows1.dtype == torch.float32 and tuple(rows1.shape) == (256, 1, frames)
    want1 = channel_mix_stats_expected(decoded, host, frames, 1)
    _same(stats1.cpu().numpy(), want1, ("decode_windows_mixed",), host)
    assert np.array_equal(rows1.cpu().numpy(), channel_mix_expected(decoded, host, frames, 1, np.float32))
    # window_levels: the statistics of the row-writing call, without the rows
    assert torch.equal(engine.window_levels(d_img, size, windows, frames, channels=1), stats1)
    assert torch.equal(engine.window_levels(d_img, size, windows, frames), stats)
    # level_dbfs: -inf for a silent row, finite elsewhere, 20 log10(rmse / 32768)
    level = level_dbfs(stats1)[:, 0]
    silent = torch.from_numpy(np.isin(host[:, 0], (2, 5))).cuda()
    assert bool((level[silent] == float("-inf")).all()) and bool(torch.isfinite(level[~silent]).all()) and bool((level[~silent] < 0).all())
    assert torch.equal(level[~silent], 20.0 * (rmse(stats1)[:, 0][~silent] / 32768.0).log10())
    # rejection sampling: levels of 2N candidates, the N loudest kept on the device, only those decoded
    keep = level_dbfs(engine.window_levels(d_img, size, windows, frames, channels=1))[:, 0].topk(128).indices
    kept = windows[keep]
    y = engine.decode_windows_mixed(d_img, size, kept, frames, channels=1)
    kept_host = kept.cpu().numpy()
    assert len(kept_host) == 128 and not np.isin(kept_host[:, 0], (2, 5)).any()  # none of the silent streams' windows
    assert np.array_equal(y.cpu().numpy(), channel_mix_expected(decoded, kept_host, frames, 1, np.float32))
    assert bool((y.abs().amax(dim=(1, 2)) > 0).all())
    # WindowDecodePlan.run's own argument checks
    hd = parse_header(bytes(d_img[0, :31].cpu().numpy()))
    plan = engine.uniform_window_decode_plan(hd, n, d_img.shape[1], size)
    try:
        for bad in (torch.zeros((256, 2, 4), dtype=torch.int32, device="cuda"), torch.zeros((256, 1, 4), dtype=torch.int64, device="cuda"),
                    torch.zeros((256, 2, 4), dtype=torch.int64), torch.zeros((256, 2, 8), dtype=torch.int64, device="cuda")[:, :, ::2]):
            with pytest.raises(ValueError):
                plan.run(d_img, windows, frames, stats=bad)
        with pytest.raises(ValueError):
            plan.run(d_img, windows, frames, rows=False)
        given = torch.full((256, 2, 4), 9, dtype=torch.int64, device="cuda")
        out, st = plan.run(d_img, windows, frames, torch.int16, stats=given)
        assert st is given and torch.equal(given, stats) and torch.equal(out, rows)
    finally:
        plan.close()


# ---- 7. errors and events -----------------------------------------------------------------------------------------------------------------
def test_argument_errors(engine, corpus):
    import torch
    images, decoded, lengths, headers, flat, table = corpus
    lib, bad, ok = engine.lib, AADApiResult.INVALID_ARGUMENT, AADApiResult.OK
    d_img = torch.from_numpy(flat).cuda()
    win = torch.tensor([[1, 0]], dtype=torch.int64, device="cuda")
    out = torch.zeros(2 * 100, dtype=torch.float32, device="cuda")
    stereo = [i for i, h in enumerate(headers) if h.num_channels == 2]
    k = stereo[0]
    # (plan, its rows per window, a stream of it, the table of window (stream, 0) at T = 100)
    plans = [(engine.channel_mix_window_decode_plan(headers, table, 2, True), 2, 1,
              channel_mix_stats_expected(decoded, [(1, 0)], 100, 2)),
             (engine.channel_mix_window_decode_plan(headers, table, 1, True), 1, 1,
              channel_mix_stats_expected(decoded, [(1, 0)], 100, 1)),
             (engine.mixed_window_decode_plan([headers[i] for i in stereo], np.ascontiguousarray(table[stereo]), True), 2, 0,
              window_stats_expected([decoded[k]], [(0, 0)], 100, 2)),
             (engine.window_decode_plan(headers[k], table[k:k + 1], True), 2, 0, window_stats_expected([decoded[k]], [(0, 0)], 100, 2))]
    for plan, channels, stream, want in plans:
        win[0, 0] = stream
        stats = torch.full((8 * 4 + 1,), PATTERN, dtype=torch.int64, device="cuda")
        sp = stats.data_ptr()
        run = lambda k, wp, frames, kind, op, tp, data=d_img.data_ptr(): lib.AADHip_WindowDecodePlanRunStats(
            plan.handle, data, k, wp, frames, kind, op, tp)
        assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), None) == bad         # a null table with N > 0
        assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, None, None) == bad
        for off in (1, 2, 4, 7):
            assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), sp + off) == bad  # not 8-byte aligned
        assert run(1, win.data_ptr(), 100, 2, None, sp) == bad                                   # sample type, rows or not
        assert run(1, win.data_ptr(), 100, -1, None, sp) == bad
        assert run(1, win.data_ptr(), 100, 2, out.data_ptr(), sp) == bad
        assert run(1, win.data_ptr(), 0, SAMPLE_INT16, out.data_ptr(), sp) == bad                # T = 0
        assert run(1, win.data_ptr(), 0, SAMPLE_INT16, None, sp) == bad
        assert run(1, None, 100, SAMPLE_INT16, out.data_ptr(), sp) == bad                        # null windows, null data
        assert run(1, win.data_ptr(), 100, SAMPLE_INT16, out.data_ptr(), sp, data=None) == bad
        assert run((1 << 62) // channels, win.data_ptr(), 1, SAMPLE_INT16, out.data_ptr(), sp) == bad  # the rows' bytes overflow
        assert run((1 << 59) // channels, win.data_ptr(), 1, SAMPLE_INT16, None, sp) == bad       # the table's alone (T < 8)
        assert lib.AADHip_WindowDecodePlanRunStats(None, d_img.data_ptr(), 1, win.data_ptr(), 100, SAMPLE_INT16, out.data_ptr(), sp) == bad
        torch.cuda.synchronize()
        assert (stats.cpu().numpy() == PATTERN).all()                                              # no failed run wrote a record
        # N = 0: OK, nothing is launched and the table is untouched
        out.fill_(-7.0)
        assert run(0, None, 100, SAMPLE_INT16, None, None, data=None) == ok
        assert run(0, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), sp) == ok
        assert run(0, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), sp + 4) == ok
        torch.cuda.synchronize()
        assert (stats.cpu().numpy() == PATTERN).all() and (out.cpu().numpy() == -7.0).all()
        # ... and the same arguments with one window run: a misaligned table one record on is refused, an aligned one is written
        assert run(1, win.data_ptr(), 100, SAMPLE_FLOAT32, out.data_ptr(), sp + 8) == ok
        torch.cuda.synchronize()
        host = stats.cpu().numpy()
        assert np.array_equal(host[1:1 + 4 * channels].reshape(1, channels, 4), want)
        assert host[0] == PATTERN and (host[1 + 4 * channels:] == PATTERN).all()
        plan.close()


def _events(engine, torch, plan, d_img, windows_np, frames, channels, want_rows, want_stats, rows):
    """AADHip_ContextSignalNextRun on a statistics run: a side stream that waits for the stop event alone sees the whole table (and
    the rows); the start event is not after the stop event; the next run leaves both alone"""
    from aad_amd.engine import HipEvent
    windows = torch.from_numpy(windows_np).cuda()
    n = len(windows_np)
    out = torch.full((n, channels, frames), 0x5A5A, dtype=torch.int16, device="cuda") if rows else None
    stats = torch.full((n, channels, 4), PATTERN, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    start, stop = HipEvent(timing=True), HipEvent(timing=True)
    engine.signal_next(stop, start=start)
    plan.run(d_img, windows, frames, torch.int16, out=out, ordered=False, stats=stats, rows=rows)  # torch's streams are not ordered ...
    stop.wait_on(side)                                                                            # ... only the side stream is
    with torch.cuda.stream(side):
        snap_stats = stats.clone()
        snap_rows = out.clone() if rows else None
    side.synchronize()
    _same(snap_stats.cpu().numpy(), want_stats, ("events", rows), windows_np)
    if rows:
        assert np.array_equal(snap_rows.cpu().numpy(), want_rows)
    start.synchronize()
    stop.synchronize()
    first = start.elapsed_ms(stop)
    assert first > 0  # the start event sits in front of the clear, the stop event behind the last kernel
    # the events were taken by that run: the next one records neither again
    again = plan.run(d_img, windows, frames, torch.int16, stats=True, rows=False)
    torch.cuda.synchronize()
    assert torch.equal(again, snap_stats)
    assert start.elapsed_ms(stop) == first


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "no_rows"])
def test_signal_next_run_events_on_a_one_kernel_run(engine, rows):
    import torch
    pcm = torch.from_numpy(synth_pcm(4, 6000, 2, seed=5)).cuda()
    d_img, size = engine.encode_uniform(pcm, make_parameter(2, 4, 1024))
    d_dec, hd = engine.decode_uniform(d_img, size)
    torch.cuda.synchronize()
    decoded = list(d_dec.cpu().numpy())
    plan = engine.uniform_window_decode_plan(hd, 4, d_img.shape[1], size)
    windows = np.array([(1, 100), (2, 3000), (3, 5900), (0, 0)] * 8, dtype=np.int64)
    _events(engine, torch, plan, d_img, windows, 3000, 2, window_expected(decoded, windows, 3000, 2),
            window_stats_expected(decoded, windows, 3000, 2), rows)
    plan.close()


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "no_rows"])
@pytest.mark.parametrize("out_channels", [1, 2])
def test_signal_next_run_events_on_a_nine_kernel_run(engine, corpus, out_channels, rows):
    import torch
    images, decoded, lengths, headers, flat, table = corpus  # nine variants: the clear and nine kernels
    d_img = torch.from_numpy(flat).cuda()
    plan = engine.channel_mix_window_decode_plan(headers, table, out_channels, True)
    frames = 3000
    windows = np.array([(s, (7 * s) % lengths[s]) for s in range(len(images))] * 8, dtype=np.int64)
    _events(engine, torch, plan, d_img, windows, frames, out_channels, channel_mix_expected(decoded, windows, frames, out_channels),
            channel_mix_stats_expected(decoded, windows, frames, out_channels), rows)
    plan.close()
