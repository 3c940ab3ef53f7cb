"""Level statistics of reverberated rows on the device (AADHip_ConvolverRunStats, aad_amd/csrc/aad_convolve_stats.hip) and the
calls built on them (Convolver.run(stats=...), Engine.window_levels_reverberated, Engine.mix_windows_reverberated).

Bar: bit for bit against tests/convolve_stats_oracle.py - v from the oracle's exact sums, the sums of a record Python integers,
`count` the closed form held against a brute force over the stream's length - with canaries on both sides of every buffer.
tests/test_convolve_stats_host.py asserts on the CPU that these inputs catch a record taken from the unclamped v, a count that
ignores the shift, sums over T instead of Le, an idle wave's stale scratch and sums left in the scratch between two items.
  * the corpora, responses and windows of tests/test_gpu_convolve.py (the three kinds of window decode plan; windows that start
    inside the lead, straddle the stream's end and start behind it; response indices outside [0, R)) at T = 257 - two blocks, the
    second with one output - and T = 1025 - five blocks, wave 0 keeps two - through Convolver.run: statistics only into a
    pre-filled table, twice; with rows in the four types, the rows those of the plain run; over spans;
  * T = 4360 on hand-made source rows through run_source and the C call: a second tile of two blocks (waves 2 and 3 idle),
    responses of 40 and 4200 taps, a row at -32768 throughout, a row whose second tile is silent, spans with Le across element
    4096, Le = 0, o >= T and an end before the second tile;
  * 2^20 + 77 rows of T = 1: a workgroup runs two items through one scratch;
  * the C call's refusals, each once, and num_windows == 0;
  * Engine.mix_windows_reverberated over the mixed-format corpus, with dry and with reverberant noise, into float32 and bfloat16,
    with noise_spans, against the composition through the oracles; the gains equal snr_gains of the oracle's tables.
Time and memory: every case below a few seconds; the item-loop case asks for 84 MB of source rows and two tables of 34 MB, every
other case for less than 8 MB."""
import numpy as np
import pytest

import convolve_oracle as co
import convolve_stats_cases as cases
import convolve_stats_oracle as so
import window_gain_oracle as go
import window_placed_oracle as po
from aad_amd.capi import AADApiResult, SAMPLE_FLOAT32, SAMPLE_INT16
from aad_amd.engine import ConvolveSource, snr_gains
from test_gpu_convolve import KINDS, PARAM_IDS, PARAMS, Setup, _convert, _expected, _float_rows
from test_gpu_resample_mix import CANARY, Bordered, _direct, _host, _spans
from test_gpu_window_resample import DTYPES, LENGTHS, _compare, corpora, engine  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(params=PARAMS, ids=PARAM_IDS)
def setup(request, engine, corpora):  # noqa: F811
    s = Setup(engine, corpora, request.param[0], request.param[1], False)
    yield s
    s.close()


def _table(torch, shape, content=CANARY["int64"]):
    return Bordered(torch, shape, "int64", content)


def _same(got, want, label=""):
    assert np.array_equal(got, want), (label, np.argwhere(got != want)[:4].tolist(), got[got != want][:4].tolist(), want[got != want][:4].tolist())


# ---- the corpora, through Convolver.run ------------------------------------------------------------------------------------------------
def test_statistics_equal_the_definition(engine, setup):  # noqa: F811
    import torch
    s = setup
    shape = (s.n, s.channels, s.frames)
    has = np.array([0 <= int(r) < len(s.responses) for r in s.index])
    assert not has.all() and (s.index < 0).any() and (s.index >= len(s.responses)).any()
    counts = so.stream_counts(LENGTHS, s.windows, s.index, s.responses, s.frames, None)
    # windows inside their stream, across its end, behind it; and windows that start inside their response's lead
    assert (counts == s.frames).any() and ((counts > 0) & (counts < s.frames)).any() and (counts[has] == 0).any()
    want = so.expected_stats(s.acc, s.qs, None, counts, has)
    assert not want[~has].any() and want[..., 2].max() >= 32767  # a clipped record among them
    assert (so.expected_stats(s.acc, s.qs, None, counts, has, clamp=False)[..., :3] != want[..., :3]).any()
    run = lambda **k: s.conv.run(s.plan, s.d_img, s.d_windows, s.frames, response=s.d_index, **k)
    table = _table(torch, (s.n, s.channels, 4))  # pre-filled: every record is overwritten
    got = run(stats=table.view, rows=False)
    assert got.data_ptr() == table.view.data_ptr()
    first = table.bits().view(np.int64)
    _same(first, want, "statistics only")
    again = run(stats=True, rows=False)
    assert np.array_equal(again.cpu().numpy(), first)  # integer sums: the same bits
    for name in DTYPES:  # with rows: those of the plain run, the records the same
        rows, table = Bordered(torch, shape, name, CANARY[name]), _table(torch, (s.n, s.channels, 4), 0x33)
        run(dtype=getattr(torch, name), out=rows.view, stats=table.view)
        _compare(rows.bits(), _convert(s.acc, s.qs, name), ("rows", name), s.windows, s.index)
        plain = run(dtype=getattr(torch, name))
        assert rows.bits().tobytes() == _host(torch, plain, name).tobytes(), name
        _same(table.bits().view(np.int64), want, name)
    spans = _spans(s.n, s.frames)
    counts = so.stream_counts(LENGTHS, s.windows, s.index, s.responses, s.frames, spans)
    want = so.expected_stats(s.acc, s.qs, spans, counts, has)
    assert (so.expected_stats(s.acc, s.qs, spans, counts, has, over_row=True) != want).any()
    table = _table(torch, (s.n, s.channels, 4))
    run(stats=table.view, rows=False, spans=torch.from_numpy(spans).cuda())
    _same(table.bits().view(np.int64), want, "spans")


# ---- tiles and atomics, on hand-made rows ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tile():
    return cases.tile_case()


def test_a_second_tile_with_idle_waves(engine, tile):  # noqa: F811
    import torch
    t = tile
    n, ch, t_src = t.rows.shape
    conv = engine.convolver(t.floats, t.delays)
    try:
        for r, (taps, q, d) in enumerate(t.responses):
            got_q, got_d, got_taps = conv.response(r)
            assert (got_q, got_d) == (q, d) and np.array_equal(got_taps, taps)
        assert conv.source_frames(t.frames) == t_src
        src = Bordered(torch, t.rows.shape, "int16", t.rows.view(np.uint16))
        source_stats = np.full((n, ch, 4), 0x77, dtype=np.int64)  # the count alone is read
        source_stats[..., 3] = t.c_src
        d_source_stats = _table(torch, (n, ch, 4), source_stats.view(np.uint64))
        source = ConvolveSource(src.view, torch.from_numpy(t.lanes.copy()).cuda(), t_src, d_source_stats.view)
        for spans in t.span_sets:
            want = so.expected_stats(t.acc, t.qs, spans, cases.counts_of(t, spans), t.has_response)
            table = _table(torch, (n, ch, 4))
            conv.run_source(source, t.frames, ch, stats=table.view, rows=False, spans=None if spans is None else torch.from_numpy(spans).cuda())
            _same(table.bits().view(np.int64), want, "spans" if spans is not None else "rows whole")
        want = so.expected_stats(t.acc, t.qs, None, cases.counts_of(t, None), t.has_response)
        for name in DTYPES:
            rows, table = Bordered(torch, (n, ch, t.frames), name, CANARY[name]), _table(torch, (n, ch, 4), 0x33)
            conv.run_source(source, t.frames, ch, getattr(torch, name), out=rows.view, stats=table.view)
            _same(rows.bits(), _convert(t.acc, t.qs, name), name)
            _same(table.bits().view(np.int64), want, name)
        # the C call, statistics only, twice into one table
        table = _table(torch, (n, ch, 4))
        for _ in range(2):
            rc = _direct(engine, engine.lib.AADHip_ConvolverRunStats, conv.handle, n, ch, src.view.data_ptr(), t_src, source.lanes.data_ptr(),
                         d_source_stats.view.data_ptr(), None, t.frames, SAMPLE_INT16, None, table.view.data_ptr())
            assert rc == AADApiResult.OK
            _same(table.bits().view(np.int64), want, "C call")
        assert np.array_equal(d_source_stats.bits().view(np.int64), source_stats) and np.array_equal(src.bits(), t.rows)
    finally:
        conv.close()


# ---- the item loop -----------------------------------------------------------------------------------------------------------------------
def test_two_items_through_one_scratch(engine):  # noqa: F811
    import torch
    h, rows, c_src = cases.item_loop_rows()
    want, _ = cases.item_loop_expected(h, rows, c_src)
    n = cases.ITEM_ROWS
    conv = engine.convolver([h], delays=[cases.ITEM_TAPS - 1])
    try:
        q, d, taps = conv.response(0)
        assert (q, d) == co.quantise(h, cases.ITEM_TAPS - 1)[1:] and np.array_equal(taps, co.quantise(h, cases.ITEM_TAPS - 1)[0])
        assert conv.source_frames(1) == cases.ITEM_TAPS
        source_stats = np.zeros((n, 1, 4), dtype=np.int64)
        source_stats[:, 0, 3] = c_src
        src = Bordered(torch, rows.shape, "int16", rows.view(np.uint16))
        source = ConvolveSource(src.view, torch.zeros((n, 2), dtype=torch.int32, device="cuda"), cases.ITEM_TAPS,
                                torch.from_numpy(source_stats).cuda())
        table = _table(torch, (n, 1, 4))
        conv.run_source(source, 1, 1, stats=table.view, rows=False)
        _same(table.bits().view(np.int64), want)
    finally:
        conv.close()


# ---- the C call's refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine):  # noqa: F811
    import torch
    lib, bad, ok = engine.lib, AADApiResult.INVALID_ARGUMENT, AADApiResult.OK
    conv = engine.convolver([[1.0], np.ones(9)])
    try:
        n, ch, frames = 4, 2, 50
        t_src = conv.source_frames(frames)
        assert t_src == frames + 8
        src = torch.full((n, ch, t_src), 7, dtype=torch.int16, device="cuda")
        lanes = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        out = Bordered(torch, (n, ch, frames), "float32", CANARY["float32"])
        stats = _table(torch, (n, ch, 4))
        src_stats = torch.full((n, ch, 4), t_src, dtype=torch.int64, device="cuda")
        spans = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        sp, ln, op, tp, ss, spn = (t.data_ptr() for t in (src, lanes, out.view, stats.view, src_stats, spans))
        f32, h = SAMPLE_FLOAT32, conv.handle

        def run_stats(**k):
            a = dict(h=h, n=n, ch=ch, sp=sp, t_src=t_src, ln=ln, ss=ss, spans=None, frames=frames, kind=f32, op=op, tp=tp)
            a.update(k)
            return lib.AADHip_ConvolverRunStats(a["h"], a["n"], a["ch"], a["sp"], a["t_src"], a["ln"], a["ss"], a["spans"], a["frames"],
                                                a["kind"], a["op"], a["tp"])

        # AADHip_ConvolverRun's errors
        for k in (dict(h=None), dict(sp=None), dict(ln=None), dict(ch=0), dict(frames=0), dict(t_src=t_src - 1), dict(kind=2), dict(kind=-1),
                  dict(sp=sp + 1), dict(ln=ln + 2), dict(op=op + 2), dict(n=1 << 62)):
            assert run_stats(**k) == bad, k
        # its own
        assert run_stats(spans=spn + 4, op=None) == bad
        assert run_stats(tp=tp + 4) == bad and run_stats(ss=ss + 4) == bad
        assert run_stats(tp=None) == bad and run_stats(ss=None) == bad
        assert run_stats(spans=spn) == bad  # rows together with spans
        assert run_stats(kind=3, op=None) == bad  # the sample type is validated without rows too
        # N * C * 32 bytes past 64 bits where N * C * T * 4 and N * C * T_src * 2 are not: T = 1 under the unit response alone
        unit = engine.convolver([[1.0]])
        try:
            many = (1 << 59) + 5
            assert unit.source_frames(1) == 1 and many * 32 >= 1 << 64 > many * 4
            assert run_stats(h=unit.handle, n=many, ch=1, frames=1, t_src=1, op=None) == bad
            assert run_stats(h=unit.handle, n=many - 10, ch=1, frames=1, t_src=1, op=None, tp=None) == bad  # a null table, sizes fine
        finally:
            unit.close()
        assert "convolver run with statistics" in engine.last_error()
        assert run_stats(n=0) == ok and run_stats(n=0, tp=None, ss=None) == ok  # no window: no launch
        engine.synchronize()
        assert (out.bits() == CANARY["float32"]).all() and (stats.bits() == CANARY["int64"]).all()
        # and the good calls are good
        assert _direct(engine, lambda: run_stats(op=None)) == ok
        want = np.tile(np.array([frames * 49, frames * 7, 7, frames], dtype=np.int64), (n, ch, 1))
        _same(stats.bits().view(np.int64), want)
        assert (out.bits() == CANARY["float32"]).all()
        assert _direct(engine, run_stats) == ok
        _same(stats.bits().view(np.int64), want)
        assert (out.bits() == np.float32(7 / 32768).view(np.uint32)).all()
    finally:
        conv.close()


# ---- engine level ------------------------------------------------------------------------------------------------------------------------
def _side(decoded, windows, index, responses, frames, channels, spans):
    """-> (float32 rows [N, C, T], stats [N, C, 4]) of one side of the mix through the oracles"""
    acc, qs = _expected(decoded, windows, index, responses, frames, channels)
    has = np.array([0 <= (0 if index is None else int(index[w])) < len(responses) for w in range(len(windows))])
    counts = so.stream_counts([len(d) for d in decoded], windows, index, responses, frames, spans)
    return _float_rows(acc, qs), so.expected_stats(acc, qs, spans, counts, has)


def _quantised(engine, floats, delays):  # noqa: F811
    conv = engine.convolver(floats, delays)
    try:
        out = []
        for r, (h, d) in enumerate(zip(floats, delays or [None] * len(floats))):
            q, delay, taps = conv.response(r)
            assert (q, delay) == co.quantise(h, d)[1:] and np.array_equal(taps, co.quantise(h, d)[0])
            out.append((taps.astype(np.int64), q, delay))
        return out
    finally:
        conv.close()


def test_mix_windows_reverberated(engine, corpora):  # noqa: F811
    import torch
    frames = 300
    images, data, table, headers, rows = corpora["mixed"]
    decoded = rows[1]
    d_img = torch.from_numpy(data).cuda()
    sizes = [len(i) for i in images]
    rng = np.random.default_rng(300)
    room = [rng.uniform(-0.5, 0.5, size=K) * np.exp(-np.arange(K) * (5.0 / K)) for K in (120, 700)]
    room[0][10], room[1][0] = 1.0, 0.8
    s_delays = [None, 0]
    hall = [np.array([0.5, 0.25, -0.125]), rng.uniform(-0.3, 0.3, size=90)]
    n_delays = [1, None]
    s_windows = np.array([(1, 0), (1, 60), (2, 900), (2, 2900), (0, 500), (3, 0), (1, 2999), (2, 3000), (4, 0), (1, 1500)], dtype=np.int64)
    n = len(s_windows)
    s_index = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 5], dtype=np.int64)  # the last one: no response, a silent signal
    n_windows = np.array([((k + 1) % 3, 41 * k) for k in range(n)], dtype=np.int64)
    n_windows[4] = (7, 0)  # no noise there: gain 0
    n_index = np.arange(n, dtype=np.int64) % 2
    spans = np.array([[(120, 40), (300, 0), (7, 293), (50, 299), (0, 0), (300, 1)][k % 6] for k in range(n)], dtype=np.int64)
    s_responses = _quantised(engine, room, s_delays)
    unit = [co.quantise([1.0])]
    unit = [(unit[0][0].astype(np.int64), unit[0][1], unit[0][2])]
    n_responses = _quantised(engine, hall, n_delays)
    s_rows, s_stats = _side(decoded, s_windows, s_index, s_responses, frames, 1, None)
    assert s_stats[:, 0, 3].tolist() == [300, 300, 300, 100, 200, 40, 1, 0, 0, 0]  # the dry row's padding mask
    cuda = lambda a: None if a is None else torch.from_numpy(a).cuda()
    for wet in (False, True):
        for noise_spans in (None, spans):
            if wet:
                n_rows, n_stats = _side(decoded, n_windows, n_index, n_responses, frames, 1, noise_spans)
            else:  # dry noise: the unit response, bit for bit window decode
                n_rows, n_stats = _side(decoded, n_windows, None, unit, frames, 1, noise_spans)
            want_gains = snr_gains(torch.from_numpy(s_stats), torch.from_numpy(n_stats), 6.0)
            assert (want_gains > 0).sum() >= n - 6 and want_gains[4] == 0 and want_gains[9] == 0
            for name in ("float32", "bfloat16"):
                got_rows, gains = engine.mix_windows_reverberated(
                    (d_img, sizes, cuda(s_windows)), (d_img, sizes, cuda(n_windows)), frames, 6.0, room, response=cuda(s_index),
                    delays=s_delays, noise_responses=hall if wet else None, noise_response=cuda(n_index) if wet else None,
                    noise_delays=n_delays if wet else None, dtype=go.torch_dtype(name), noise_spans=cuda(noise_spans))
                assert got_rows.dtype == go.torch_dtype(name) and got_rows.shape == (n, 1, frames)
                assert torch.equal(gains.cpu(), want_gains), (wet, noise_spans is not None, name)
                first = po.placed_expected(s_rows, None, np.ones(n, dtype=np.float32), name)
                want = po.placed_expected(n_rows, noise_spans, gains.cpu().numpy(), name, first)  # with the RETURNED gains
                assert (want != first).any()
                _compare(_host(torch, got_rows, name), want, ("mix", wet, noise_spans is not None, name), s_windows, s_index)
    levels = engine.window_levels_reverberated(d_img, sizes, cuda(n_windows), frames, hall, response=cuda(n_index), delays=n_delays,
                                               spans=cuda(spans))
    assert np.array_equal(levels.cpu().numpy(), n_stats)
    got_rows, levels = engine.decode_windows_reverberated(d_img, sizes, cuda(s_windows), frames, room, response=cuda(s_index),
                                                          delays=s_delays, return_stats=True)
    assert np.array_equal(levels.cpu().numpy(), s_stats) and np.array_equal(_host(torch, got_rows, "float32"), s_rows.view(np.uint32))
