"""The convolve stage's FIR kernels (aad_amd/csrc/aad_convolve.hip, aad_convolve_tile.hip.h) at the launch geometry the value tests
of tests/test_gpu_convolve.py do not reach, through the C calls on hand-made int16 source rows and lanes (AADHip_ConvolverRun,
...RunGain) and through Convolver.run_source: no codec, numpy's convolve and device memory.

  test                          geometry                                                         what a wrong kernel would do
  ----------------------------  ---------------------------------------------------------------  ------------------------------------
  test_source_placement         T = 257, 1025, K = 1, 64, 65, 1000, 4200; the source pointer at   a vector load that assumes
                                both parities, the pitch T_src + 0, 1, 37 with the rails behind   alignment, a bound or a pitch taken
                                T_src, tables and outputs off 16-byte alignment                   from T_src: other bytes
  test_shift_past_the_lead      pitch T_src + 37, shifts lead + 1, + 36, + 37, the pitch,         the surplus not read as source; a
                                2^31 - 1, 2^31, 2^32 - 1                                          32-bit j wraps back into the row
  test_item_loop                2^20 + 1024 rows of T = 9: 1024 workgroups take two items,        a kept response, shift or
                                every ordered pair of {none, K = 1, 40, 1000, 4082}, in the       accumulator, a barrier lost between
                                gain runs with empty spans and the span (4, 5)                    items or pieces
  test_index_limit              T = 2^31 + 4096 + 77, two rows, response [3, -2, 1]               n, n0 or Le - n0 signed or wrapped
  test_past_4_gib               1 048 800 rows of T = 4099, odd pitch above T_src, pointer at     a narrowed row offset: another
                                parity 1: rows past 2^32 elements of source and output            row's data, in bounds

Every buffer lies between canaries, every comparison is bit for bit: rows with a response against
tests/convolve_rows_oracle.py (held to the definition, and to catching each of these mistakes, by
tests/test_convolve_geometry_host.py), the bulk rows of the large cases - the response {1.0}: the output IS the source slice,
[3, -2, 1]: a closed form - on the device, over every element."""
import numpy as np
import pytest

import convolve_oracle as co
import convolve_rows_oracle as cr
from aad_amd.capi import AADApiResult, WINDOW_GAIN_ADD, WINDOW_GAIN_STORE
from aad_amd.engine import ConvolveSource
from test_gpu_convolve import KINDS
from test_gpu_resample_geometry import GIB, Fence, _gains, _skewed, _source_on_device, big_engine  # noqa: F401
from test_gpu_resample_mix import _direct
from test_gpu_window_resample import engine  # noqa: F401

pytestmark = pytest.mark.gpu


def _need(torch, need, what):
    """the skip of every big test: `need` GiB and 8 GiB of headroom"""
    free, _ = torch.cuda.mem_get_info()
    if free < (need + 8) * GIB:
        pytest.skip("needs %d GiB of free device memory (%s) plus 8 GiB headroom, %.1f GiB free" % (need, what, free / GIB))


class Rig:
    """a convolver whose responses the library quantised as the oracle does"""

    def __init__(self, engine, hs, delays):  # noqa: F811
        self.engine, self.conv = engine, engine.convolver(hs, delays)
        self.responses = cr.quantised(hs, [None] * len(hs) if delays is None else delays)
        for r, (taps, q, d) in enumerate(self.responses):
            got = self.conv.response(r)
            assert got[:2] == (q, d) and np.array_equal(got[2], taps), r

    def close(self):
        self.conv.close()


def _launch(rig, run, n, channels, d_src, d_lanes, d_spans, d_gains, frames, out):
    kind, name, add = run
    e, lib = rig.engine, rig.engine.lib
    common = (rig.conv.handle, n, channels, d_src.data_ptr(), d_src.shape[1], d_lanes.data_ptr())
    if kind == "rows":
        rc = _direct(e, lib.AADHip_ConvolverRun, *common, frames, KINDS[name], out.view.data_ptr())
    else:
        rc = _direct(e, lib.AADHip_ConvolverRunGain, *common, d_spans.data_ptr(), frames, KINDS[name], out.view.data_ptr(),
                     d_gains.data_ptr(), WINDOW_GAIN_ADD if add else WINDOW_GAIN_STORE)
    assert rc == AADApiResult.OK, (run, e.last_error())


def _first_bad(got, want):
    return (cr.bit_view(got) != cr.bit_view(want)).nonzero()[:6].cpu().numpy()


class Batch:
    """One launch geometry: N windows x C rows of T outputs over d_src [N * C, pitch] on the device.
    special: the rows (sorted indices) whose expectation is the numpy FIR over their downloaded source rows, None: all of them;
    every other row has the unit response and is held to its source slice on the device, `chunk` rows at a time."""

    def __init__(self, torch, rig, frames, channels, lanes, d_src, spans, gains, special=None, chunk=None, skew=0, front=16):
        self.torch, self.rig, self.frames, self.channels, self.front = torch, rig, frames, channels, front
        self.n, self.rows = len(lanes), len(lanes) * channels
        self.lanes, self.d_src, self.pitch = lanes, d_src, d_src.shape[1]
        assert d_src.shape[0] == self.rows and d_src.stride(0) == self.pitch and d_src.stride(1) == 1
        assert self.pitch >= rig.conv.source_frames(frames)
        self.gains = gains.astype(np.float32)
        self.d_lanes = _skewed(torch, cr.device_lanes(lanes), skew)
        self.d_spans = _skewed(torch, spans.astype(np.int64), skew)
        self.d_gains = _skewed(torch, self.gains, skew)
        self.le, self.o = cr.clipped_rows(spans, self.n, frames, channels)
        self.bulk = special is not None
        self.special = np.arange(self.rows, dtype=np.int64) if special is None else np.asarray(special, dtype=np.int64)
        self.chunk = chunk or self.rows
        sp = self.special
        self.d_special = torch.from_numpy(sp).cuda()
        self.src_special, self.lanes_special = d_src[self.d_special].cpu().numpy(), lanes[sp // channels]
        self.acc = cr.expected_acc(self.src_special, self.lanes_special, rig.responses, frames, 1)[:, 0]  # each special row a window
        self.qs = cr.lane_scales(self.lanes_special, rig.responses)
        if self.bulk:
            assert rig.responses[0][0].tolist() == list(cr.UNIT_TAPS) and rig.responses[0][1:] == (cr.UNIT_Q, 0)
            rest = np.ones(self.n, dtype=bool)
            rest[sp // channels] = False
            assert (lanes[rest, 0] == 0).all() and lanes[rest, 1].max() <= 3 and 3 + frames <= self.pitch
            self.d_shift = torch.from_numpy(np.repeat(lanes[:, 1], channels)).cuda()
            self.d_le, self.d_o = torch.from_numpy(self.le).cuda(), torch.from_numpy(self.o).cuda()
            self.d_row_gain = torch.from_numpy(np.repeat(self.gains, channels)).cuda()

    def _elements(self, rows):
        """the output buffer's element index of every element of the rows `rows` (an int64 tensor)"""
        return rows[:, None] * self.frames + self.torch.arange(self.frames, dtype=self.torch.int64, device=rows.device)[None, :]

    def _bulk_expected(self, run, r0, r1, old):
        """rows r0 ... r1 - 1 as rows of the unit response, on the device"""
        torch = self.torch
        kind, name, add = run
        T = self.frames
        src, shift = self.d_src[r0:r1], self.d_shift[r0:r1]
        v16 = src[:, 0:T]
        for s in (1, 2, 3):
            v16 = torch.where((shift == s)[:, None], src[:, s:s + T], v16)
        if kind == "rows":
            return v16 if name == "int16" else (v16.to(torch.float32) * 2.0 ** -15).to(cr.torch_dtype(name))
        return cr.placed_rows(v16.to(torch.float32) * 2.0 ** -15, self.d_le[r0:r1], self.d_o[r0:r1], self.d_row_gain[r0:r1], name,
                              old if add else None)

    def run(self, run):
        """launch, canaries, and every element against its expectation -> the bytes written (small batches)"""
        torch = self.torch
        kind, name, add = run
        T = self.frames
        out = Fence(torch, self.rows * T, name, self.front)
        if add:
            for r0 in range(0, self.rows, self.chunk):
                r1 = min(r0 + self.chunk, self.rows)
                out.view[r0 * T:r1 * T] = cr.old_pattern(torch.arange(r0 * T, r1 * T, dtype=torch.int64, device="cuda"), name)
        _launch(self.rig, run, self.n, self.channels, self.d_src, self.d_lanes, self.d_spans, self.d_gains, T, out)
        out.check()
        sp = self.special
        old_sp = cr.old_pattern(self._elements(torch.from_numpy(sp)), name) if add else None
        want_rows = cr.run_expected(run, self.acc, self.qs, self.le[sp], self.o[sp], self.gains[sp // self.channels], old_sp).cuda()
        for r0 in range(0, self.rows, self.chunk):
            r1 = min(r0 + self.chunk, self.rows)
            a, b = np.searchsorted(sp, [r0, r1])
            if self.bulk:
                old = cr.old_pattern(torch.arange(r0 * T, r1 * T, dtype=torch.int64, device="cuda"), name).view(r1 - r0, T) if add else None
                rows = self._bulk_expected(run, r0, r1, old)
                rows[self.d_special[a:b] - r0] = want_rows[a:b]
            else:
                assert b - a == r1 - r0
                rows = want_rows[a:b]
            got = out.view[r0 * T:r1 * T].view(r1 - r0, T)
            if not torch.equal(cr.bit_view(got), cr.bit_view(rows)):
                bad = _first_bad(got, rows)
                bad[:, 0] += r0
                raise AssertionError("%s: rows differ, first at (row, element) %s; lanes %s" %
                                     (cr.run_id(run), bad.tolist(), self.lanes[bad[:, 0] // self.channels].tolist()))
        if self.rows * T > 1 << 24:
            return None
        return bytes(cr.bit_view(out.view).cpu().numpy().tobytes())


def _placed(torch, host, parity):
    """int16 rows [R, pitch] on the device, the first `parity` int16 into a fresh allocation"""
    big = torch.empty(host.size + parity, dtype=torch.int16, device="cuda")
    d_src = big[parity:].view(*host.shape)
    d_src.copy_(torch.from_numpy(host))
    assert d_src.data_ptr() % 4 == 2 * parity
    return d_src


# ---- a. source placement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", cr.PLACE_FRAMES)
def test_source_placement(engine, frames):  # noqa: F811
    import torch
    C_ = 2
    rig = Rig(engine, *cr.place_responses())
    try:
        t_src = rig.conv.source_frames(frames)
        assert t_src == co.source_frames(frames, rig.responses) and t_src % 2 == 0
        lanes = cr.place_lanes(rig.responses)
        n = len(lanes)
        rng = np.random.default_rng(frames)
        base = cr.source_rows(rng, n * C_, t_src)
        spans, gains = cr.spans_for(n, frames), _gains(rng, n)
        written, acc = {}, None
        for parity in (0, 1):
            for extra in cr.PLACE_EXTRAS:
                d_src = _placed(torch, cr.pitched(base, t_src, extra), parity)  # the rails behind T_src: no output may read them
                b = Batch(torch, rig, frames, C_, lanes, d_src, spans, gains, skew=1, front=17)
                assert b.d_gains.data_ptr() % 16 == 4 and b.d_lanes.data_ptr() % 16 == 4 and b.d_spans.data_ptr() % 16 == 8
                acc = b.acc if acc is None else acc
                assert np.array_equal(b.acc, acc)  # the definition over the whole pitch: the same rows at every pitch
                written[parity, extra] = {cr.run_id(run): b.run(run) for run in cr.RUNS}
                source = ConvolveSource(d_src.view(n, C_, -1), b.d_lanes.view(n, 2), t_src + extra)
                for name in cr.DTYPES:  # and through the Python call: the same bytes
                    out = Fence(torch, n * C_ * frames, name, 17)
                    assert out.view.data_ptr() % 16 == (4 if name == "float32" else 2)
                    rig.conv.run_source(source, frames, C_, cr.torch_dtype(name), out=out.view.view(n, C_, frames))
                    engine.synchronize()
                    out.check()
                    assert bytes(cr.bit_view(out.view).cpu().numpy().tobytes()) == written[parity, extra]["rows-%s" % name], name
        assert (acc != 0).any(axis=1).sum() >= 2 * (n - 1)
        first = written[0, 0]
        assert all(v is not None and len(v) > 0 for v in first.values()) and len(first) == 10
        for key, other in written.items():
            for name, data in other.items():
                assert data == first[name], ("the placement changes the bytes", key, name)
    finally:
        rig.close()


# ---- b. shifts past the lead -------------------------------------------------------------------------------------------------------------
PAST_RUNS = [("rows", "int16", False), ("rows", "float32", False), ("gain", "float16", True)]


@pytest.mark.parametrize("frames", cr.PLACE_FRAMES)
def test_shift_past_the_lead(engine, frames):  # noqa: F811
    import torch
    C_ = 2
    rig = Rig(engine, *cr.place_responses())
    try:
        t_src = rig.conv.source_frames(frames)
        pitch = t_src + cr.SURPLUS
        lanes = cr.past_lead_lanes(rig.responses, pitch)
        n = len(lanes)
        rng = np.random.default_rng(37 + frames)
        host = cr.pitched(cr.source_rows(rng, n * C_, t_src), t_src, cr.SURPLUS)
        gains = _gains(rng, n)
        for parity in (0, 1):
            b = Batch(torch, rig, frames, C_, lanes, _placed(torch, host, parity), cr.spans_for(n, frames), gains, skew=1, front=17)
            # the surplus is read: the rows differ from those of a row that ends at T_src; the huge shifts give rows of zeros
            cut = b.src_special.copy()
            cut[:, t_src:] = 0
            short = cr.expected_acc(cut, b.lanes_special, rig.responses, frames, 1)[:, 0]
            lead = cr.leads(rig.responses)
            for row, (r, shift) in enumerate(b.lanes_special.tolist()):
                if shift >= (1 << 31) - 1:
                    assert not b.acc[row].any()
                elif (r == 4 and shift <= lead[4] + cr.SURPLUS) or (shift == pitch and lead[r] > 0):
                    assert (co.element_bits(b.acc[row], int(b.qs[row]), "float32") != co.element_bits(short[row], int(b.qs[row]), "float32")).any()
            written = [b.run(run) for run in PAST_RUNS]
            assert all(written)
    finally:
        rig.close()


# ---- c. the item loop --------------------------------------------------------------------------------------------------------------------
def test_item_loop(engine):  # noqa: F811
    import torch
    _need(torch, 10, "the source batch, 8.6 GB")
    T, E, G = cr.ITEM_FRAMES, cr.ITEM_EXTRA, cr.GRID
    rig = Rig(engine, *cr.item_responses())
    d_src = b = None
    try:
        rows = cr.item_rows()
        t_src = rig.conv.source_frames(T)
        assert t_src == T + max(k for k in cr.ITEM_KINDS if k) - 1
        lanes, designed = cr.item_lanes(rig.responses)
        rng = np.random.default_rng(2 ** 20)
        sample = rng.choice(np.setdiff1d(np.arange(rows), designed), size=4096, replace=False)
        special = np.sort(np.concatenate([designed, sample]))
        d_src = _source_on_device(torch, rows, t_src, seed=77)
        gains = cr.bulk_gains(rng, rows)  # exact in the bulk
        gains[special] = rng.uniform(-2.0, 2.0, size=len(special))
        b = Batch(torch, rig, T, 1, lanes, d_src, cr.spans_for(rows, T), gains, special=special)
        # before the device is asked: a designed row with a response is not silent, in int16 and in float32, and the second item
        # of a workgroup differs from what the first item's response and shift give over its row (the first 100 workgroups: four
        # of every ordered pair) - a kept response or shift cannot pass
        at = np.searchsorted(special, designed)
        acc, lane, qs = b.acc[at], b.lanes_special[at], b.qs[at]
        for k in range(1, len(cr.ITEM_KINDS)):
            mine = lane[:, 0] == k
            assert mine.sum() >= 2 * 32 * 5
            for name in ("int16", "float32"):
                assert (co.element_bits(acc[mine], int(qs[mine][0]), name) != 0).any(axis=1).all(), (k, name)
        assert not acc[lane[:, 0] == cr.NO_RESPONSE].any()
        first, second = lane[:100], lane[E:E + 100]
        kept = (first[:, 0] != cr.NO_RESPONSE) & (first != second).any(axis=1)
        stale = cr.expected_acc(b.src_special[at][E:E + 100][kept], first[kept], rig.responses, T, 1)[:, 0]
        q2 = qs[E:E + 100][kept]
        for i in range(len(stale)):
            for name in ("int16", "float32"):
                assert (co.element_bits(stale[i], int(q2[i]), name) != co.element_bits(acc[E:E + 100][kept][i], int(q2[i]), name)).any()
        assert kept.sum() >= 70
        for run in cr.RUNS:
            b.run(run)
    finally:
        rig.close()
        del d_src, b
        torch.cuda.empty_cache()


# ---- d. the 2^31 limit -------------------------------------------------------------------------------------------------------------------
LIMIT_RUNS = [("rows", "int16", False), ("rows", "float32", False), ("gain", "float32", False)]


def test_index_limit(big_engine):
    import torch
    _need(torch, 36, "the source rows 8, float32 rows 16, a chunk's expectation 12")
    T, step = cr.LIMIT_FRAMES, 1 << 28
    rig = Rig(big_engine, [cr.RECURRENCE_RESPONSE], None)
    d_src = out = None
    try:
        assert (tuple(rig.responses[0][0].tolist()),) + rig.responses[0][1:] == (cr.RECURRENCE_TAPS, cr.RECURRENCE_Q, cr.RECURRENCE_DELAY)
        t_src = rig.conv.source_frames(T)
        assert t_src == T + 2
        lanes = np.array([(0, s) for s in cr.LIMIT_SHIFTS], dtype=np.int64)
        spans = np.array([(T - o, o) for o in cr.LIMIT_OFFSETS], dtype=np.int64)  # each ends at the last output
        gains = np.array([-0.5, 2.0], dtype=np.float32)
        d_src = _source_on_device(torch, 2, t_src, seed=31)
        d_lanes, d_spans, d_gains = (torch.from_numpy(v).cuda() for v in (cr.device_lanes(lanes), spans, gains))
        for run in LIMIT_RUNS:
            kind, name, _ = run
            out = Fence(torch, 2 * T, name)
            _launch(rig, run, 2, 1, d_src, d_lanes, d_spans, d_gains, T, out)
            out.check()
            for r in range(2):
                o, g = (cr.LIMIT_OFFSETS[r], float(gains[r])) if kind == "gain" else (0, 1.0)
                row = out.view[r * T:(r + 1) * T]
                assert not bool(cr.bit_view(row[:o]).any()), (run, r, "+0 in front of the span")
                for lo in range(0, T - o, step):
                    hi = min(lo + step, T - o)
                    v = cr.recurrence(d_src[r], cr.LIMIT_SHIFTS[r], T, lo, hi, xp=torch, device="cuda")
                    want = cr.recurrence_int16(v, torch).to(torch.int16) if name == "int16" else v.to(torch.float32) * 2.0 ** -15 * g
                    del v
                    got = row[o + lo:o + hi]
                    if not torch.equal(cr.bit_view(got), cr.bit_view(want)):
                        raise AssertionError("%s: row %d differs, first at crop indices %s" %
                                             (cr.run_id(run), r, (_first_bad(got, want)[:, 0] + lo).tolist()))
                    del want
            out = None
            torch.cuda.empty_cache()
    finally:
        rig.close()
        del d_src, out
        torch.cuda.empty_cache()


# ---- e. past 4 GiB -----------------------------------------------------------------------------------------------------------------------
BIG_RUNS = [("rows", "int16", False), ("rows", "float32", False), ("gain", "float32", False), ("gain", "bfloat16", True)]


def test_past_4_gib(big_engine):
    import torch
    _need(torch, 30, "the source batch 8.2, float32 rows 16, a chunk's expectation and its index tensors")
    T, C_, n = cr.BIG_FRAMES, 2, cr.BIG_WINDOWS
    rows, pitch = n * C_, cr.big_pitch()
    rig = Rig(big_engine, *cr.big_responses())
    d_src = b = None
    try:
        assert rig.conv.source_frames(T) == pitch - 2
        witnesses = cr.big_witness_windows()
        rng = np.random.default_rng(4099)
        lanes = np.empty((n, 2), dtype=np.int64)
        lanes[:, 0], lanes[:, 1] = 0, np.arange(n) % 4
        lead = cr.leads(rig.responses)
        for k, w in enumerate(witnesses.tolist()):
            r = 1 + k % (len(rig.responses) - 1)
            lanes[w] = (r, rng.integers(0, lead[r] + 3))
        special = np.sort(np.concatenate([witnesses * 2, witnesses * 2 + 1]))
        d_src = _source_on_device(torch, rows, pitch, seed=4099, parity=1)
        assert d_src.data_ptr() % 4 == 2 and rows * pitch > 1 << 32 and rows * T > 1 << 32
        assert bool((d_src[1:, :32] != d_src[:-1, :32]).any(dim=1).all())  # neighbouring rows have different data
        gains = cr.bulk_gains(rng, n)
        gains[witnesses] = rng.uniform(-2.0, 2.0, size=len(witnesses))
        b = Batch(torch, rig, T, C_, lanes, d_src, cr.spans_for(n, T), gains, special=special, chunk=1 << 14)
        assert (b.acc != 0).any(axis=1).all() and (b.acc[:, cr.TILE:] != 0).any(axis=1).all()  # the tile of three outputs has data
        for run in BIG_RUNS:
            b.run(run)
            torch.cuda.empty_cache()
    finally:
        rig.close()
        del d_src, b
        torch.cuda.empty_cache()
