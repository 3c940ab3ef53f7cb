"""The resample stage's FIR kernels (aad_amd/csrc/aad_resample.hip, aad_resample_wide.hip, aad_resample_tile.hip.h) at the launch
geometry the value tests do not reach, through the C calls on hand-made source rows, lanes and source statistics
(AADHip_ResamplerRun, ...RunGain, ...RunStats): no codec, a numpy FIR and device memory.

  test                          geometry                                                         what a wrong kernel would do
  ----------------------------  ---------------------------------------------------------------  ------------------------------------
  test_full_tiles               T = 4097: four full tiles and one output; a tile n0 > 0 spans     a span short for its tile: the
                                floor(1023 M / L) + 1 source frames; a row that ends mid-tile;    last output of a tile reads LDS
                                two more resamplers whose widest bank ends in non-zero taps       that was never staged
  test_source_alignment         T = 257, 1025; source pointer and row pitch at both parities,     `front` wrong: every tap one
                                outputs and tables off 16-byte alignment                          frame off in the odd rows
  test_item_loop                2 * 2^20 + 1024 rows of T = 9: 1024 workgroups take three         a kept or stale bank, a missing
                                items, every ordered triple of {no bank, resident, gathered}      barrier, scratch of the last item
  test_index_limit              (T - 1) M just below 2^31: T = 196 423 of 1025/10933 and          32-bit n M, i, p wrap; ~1500 tiles
                                T = 1 573 249 of 1024/1365, every output against the FIR          contend for one record
  test_past_4_gib               1 048 400 rows of T = 4099, C = 2: outputs past 2^32 elements,    a narrowed row offset writes
                                2^34 bytes; rows x tiles past 2^22                                another row, in bounds

Each test runs a plain resampler and wide ones (the ratio sets of tests/test_gpu_resample_wide.py: rounds of 64, 128 and 256),
all 15 FIR kernels of each in the first three, every buffer between canaries, every comparison bit for bit: rows with a bank
against tests/resample_rows_oracle.py (held to the definition by tests/test_resample_geometry_host.py, as are the case tables),
the bulk rows of the two large cases - identity bank, whose row is [16384, 0]: the output IS the source slice - against that
slice on the device, over every element."""
import ctypes as C

import numpy as np
import pytest

import resample_oracle as ro
import resample_rows_oracle as rr
import test_gpu_resample_mix as mix
import test_gpu_resample_wide as wide_tests
from aad_amd.capi import AADApiResult, WINDOW_GAIN_ADD, WINDOW_GAIN_STORE
from test_gpu_window_resample import engine  # noqa: F401

pytestmark = pytest.mark.gpu

GIB = 1 << 30
CANARY = {"int16": 0x5A5A, "float32": -7.0, "float16": -7.0, "bfloat16": -7.0, "int64": 0x5A5A5A5A5A5A5A5A}
BEFORE = {"int16": 0x1D2B, "float32": float("nan"), "float16": float("nan"), "bfloat16": float("nan"), "int64": 0x33}
NAMES = sorted(rr.resamplers())


def test_the_wide_sets_are_those_of_the_wide_tests():
    assert rr.WIDE_SETS == wide_tests.SETS and rr.RESIDENT == wide_tests.RESIDENT


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
class Fence:
    """`count` elements on the device behind `front` canary elements and in front of 16"""

    def __init__(self, torch, count, name, front=16):
        self.torch, self.name, self.front, self.count = torch, name, front, count
        self.big = torch.empty(count + front + 16, dtype=rr.torch_dtype(name), device="cuda")
        self.big[:front].fill_(CANARY[name])
        self.big[front + count:].fill_(CANARY[name])
        self.view = self.big[front:front + count]
        step = 1 << 28
        for a in range(0, count, step):
            self.view[a:a + step].fill_(BEFORE[name])

    def check(self):
        border = self.torch.cat([self.big[:self.front], self.big[self.front + self.count:]])
        assert bool((border == CANARY[self.name]).all()), "wrote outside its buffer"


def _skewed(torch, array, skew):
    """a numpy array on the device, `skew` elements into its allocation: element-aligned, with skew = 1 not 16-byte aligned"""
    flat = torch.from_numpy(np.ascontiguousarray(array)).reshape(-1)
    big = torch.empty(flat.numel() + skew, dtype=flat.dtype, device="cuda")
    big[skew:].copy_(flat)
    return big[skew:]


def _source_on_device(torch, rows, pitch, seed, parity=0):
    """random int16 rows with the rails sprinkled in, generated on the device: -> [rows, pitch] view, `parity` int16 into its
    allocation"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    count = rows * pitch
    big = torch.empty(count + parity, dtype=torch.int16, device="cuda")
    step = 1 << 28
    for a in range(0, count, step):
        n = min(step, count - a)
        v = torch.randint(-32768, 32768, (n,), dtype=torch.int16, device="cuda", generator=g)
        r = torch.randint(0, 24, (n,), dtype=torch.int8, device="cuda", generator=g)
        v.masked_fill_(r == 0, 32767).masked_fill_(r == 1, -32768)
        big[parity + a:parity + a + n] = v
        del v, r
    return big[parity:].view(rows, pitch)


def _source_rows(rng, rows, t_src):
    x = rng.integers(-32768, 32768, size=(rows, t_src)).astype(np.int16)
    rail = rng.integers(0, 24, size=x.shape)
    x[rail == 0], x[rail == 1] = 32767, -32768
    return x


# ---- a resampler and a batch -----------------------------------------------------------------------------------------------------------
class Rig:
    def __init__(self, engine, ratios, wide):  # noqa: F811
        self.engine, self.ratios, self.wide = engine, ratios, wide
        self.res = engine.resampler(ratios, [list(range(len(ratios)))], wide=wide)
        self.banks = [self.res.bank(r) for r in range(len(ratios))]
        assert [(L, M) for L, M, _ in self.banks] == list(ratios)
        assert [h.shape[1] for _, _, h in self.banks] == [ro.taps(L, M) for L, M in ratios]

    def close(self):
        self.res.close()


class Batch:
    """One launch geometry: N windows x C rows of T outputs over d_src [N * C, source_frames] on the device.
    special: the rows (sorted indices) whose expectation is the numpy FIR over their downloaded source rows, None: all of them;
    every other row has the identity bank and is held to its source slice on the device, `chunk` rows at a time."""

    def __init__(self, torch, rig, frames, channels, lanes, d_src, c_src, spans, gains, special=None, chunk=None, skew=0, front=16):
        self.torch, self.rig, self.frames, self.channels, self.front = torch, rig, frames, channels, front
        self.n, self.rows = len(lanes), len(lanes) * channels
        self.lanes, self.d_src, self.source_frames = lanes, d_src, d_src.shape[1]
        assert d_src.shape[0] == self.rows and d_src.stride(0) == self.source_frames
        self.needed = rig.res.source_frames(frames)
        assert self.source_frames >= self.needed
        self.spans, self.gains, self.c_src = spans, gains.astype(np.float32), c_src
        self.d_lanes = _skewed(torch, lanes.astype(np.int32), skew)
        self.d_spans = _skewed(torch, spans.astype(np.int64), skew)
        self.d_gains = _skewed(torch, self.gains, skew)
        stats = np.full((self.rows, 4), 0x77, dtype=np.int64)  # the count alone is read
        stats[:, 3] = c_src
        self.d_source_stats = _skewed(torch, stats, skew)
        self.le, self.o = rr.clipped_rows(spans, self.n, frames, channels)
        self.bulk = special is not None
        self.special = np.arange(self.rows, dtype=np.int64) if special is None else np.asarray(special, dtype=np.int64)
        self.chunk = chunk or self.rows
        sp = self.special
        self.d_special = torch.from_numpy(sp).cuda()
        src = d_src[self.d_special].cpu().numpy()
        lanes_sp = lanes[sp // channels]
        self.acc = rr.expected_acc(src, lanes_sp, rig.banks, frames, 1)[:, 0]  # each special row a window of one channel
        self.src_special, self.lanes_special = src, lanes_sp
        self.counts_full = rr.output_counts(c_src[sp], self.source_frames, lanes_sp, rig.banks, frames, None, 1)[:, 0]
        self.counts_span = rr.output_counts(c_src[sp], self.source_frames, lanes_sp, rig.banks, frames, spans[sp // channels], 1)[:, 0]
        if self.bulk:
            identity = rig.ratios.index((1, 1))
            L, M, h = rig.banks[identity]
            assert (L, M) == (1, 1) and h.tolist() == [[16384, 0]]  # the bulk's output is its source slice for this bank alone
            rest = np.ones(self.n, dtype=bool)
            rest[sp // channels] = False
            assert (lanes[rest, 0] == identity).all() and lanes[rest, 1].max() <= 3 and 3 + frames <= self.source_frames
            self.d_shift = torch.from_numpy(np.repeat(lanes[:, 1], channels)).cuda()
            self.d_le, self.d_o = torch.from_numpy(self.le).cuda(), torch.from_numpy(self.o).cuda()
            self.d_row_gain = torch.from_numpy(np.repeat(self.gains, channels)).cuda()
            self.d_c_src = torch.from_numpy(np.ascontiguousarray(c_src)).cuda()

    # -- the run ----------------------------------------------------------------------------------------------------------------------
    def launch(self, run, out, table):
        kind, name, flag = run
        lib, e, h = self.rig.engine.lib, self.rig.engine, self.rig.res.handle
        sample = mix.KINDS[name or "int16"]
        op = None if out is None else out.view.data_ptr()
        common = (h, self.n, self.channels, self.d_src.data_ptr(), self.source_frames, self.d_lanes.data_ptr())
        if kind == "rows":
            rc = mix._direct(e, lib.AADHip_ResamplerRun, *common, self.frames, sample, op)
        elif kind == "gain":
            rc = mix._direct(e, lib.AADHip_ResamplerRunGain, *common, self.d_spans.data_ptr(), self.frames, sample, op,
                             self.d_gains.data_ptr(), WINDOW_GAIN_ADD if flag else WINDOW_GAIN_STORE)
        else:
            rc = mix._direct(e, lib.AADHip_ResamplerRunStats, *common, self.d_source_stats.data_ptr(),
                             self.d_spans.data_ptr() if flag else None, self.frames, sample, op, table.view.data_ptr())
        assert rc == AADApiResult.OK, (run, e.last_error())

    def _elements(self, rows):
        """the output buffer's element index of every element of the rows `rows` (an int64 tensor)"""
        return rows[:, None] * self.frames + self.torch.arange(self.frames, dtype=self.torch.int64, device=rows.device)[None, :]

    def _bulk_expected(self, run, r0, r1, old):
        """rows r0 ... r1 - 1 as identity rows, on the device -> (rows or None, records or None)"""
        torch = self.torch
        kind, name, flag = run
        T = self.frames
        src, shift = self.d_src[r0:r1], self.d_shift[r0:r1]
        v16 = src[:, 0:T]
        for s in (1, 2, 3):
            v16 = torch.where((shift == s)[:, None], src[:, s:s + T], v16)
        whole = torch.full((r1 - r0,), T, dtype=torch.int64, device="cuda")
        rows = records = None
        if kind == "rows" or (kind == "stats" and name is not None):
            rows = v16 if name == "int16" else (v16.to(torch.float32) * 2.0 ** -15).to(rr.torch_dtype(name))
        elif kind == "gain":
            rows = rr.placed_rows(v16.to(torch.float32) * 2.0 ** -15, self.d_le[r0:r1], self.d_o[r0:r1], self.d_row_gain[r0:r1], name,
                                  old if flag else None)
        if kind == "stats":
            le = self.d_le[r0:r1] if flag else whole
            records = rr.row_records(v16, le, rr.identity_counts(self.d_c_src[r0:r1], self.source_frames, shift, le))
        return rows, records

    def run(self, run):
        """launch, canaries, and every element against its expectation -> the bytes written (small batches)"""
        torch = self.torch
        kind, name, flag = run
        T = self.frames
        add = kind == "gain" and flag
        out = table = None
        if name is not None:
            out = Fence(torch, self.rows * T, name, self.front)
        if kind == "stats":
            table = Fence(torch, self.rows * 4, "int64", self.front)
        if add:
            for r0 in range(0, self.rows, self.chunk):
                r1 = min(r0 + self.chunk, self.rows)
                out.view[r0 * T:r1 * T] = rr.old_pattern(torch.arange(r0 * T, r1 * T, dtype=torch.int64, device="cuda"), name)
        self.launch(run, out, table)
        for f in (out, table):
            if f is not None:
                f.check()
        sp = self.special
        old_sp = rr.old_pattern(self._elements(torch.from_numpy(sp)), name) if add else None
        gain_sp = self.gains[sp // self.channels]
        want_rows, want_rec = rr.run_expected(run, self.acc, self.le[sp], self.o[sp], gain_sp, old_sp, self.counts_full, self.counts_span)
        want_rows = None if want_rows is None else want_rows.cuda()
        want_rec = None if want_rec is None else want_rec.cuda()
        for r0 in range(0, self.rows, self.chunk):
            r1 = min(r0 + self.chunk, self.rows)
            a, b = np.searchsorted(sp, [r0, r1])
            local = self.d_special[a:b] - r0
            rows = records = None
            if self.bulk:
                old = rr.old_pattern(torch.arange(r0 * T, r1 * T, dtype=torch.int64, device="cuda"), name).view(r1 - r0, T) if add else None
                rows, records = self._bulk_expected(run, r0, r1, old)
            if out is not None:
                if rows is None:
                    assert b - a == r1 - r0
                    rows = want_rows[a:b]
                else:
                    rows[local] = want_rows[a:b]
                got = out.view[r0 * T:r1 * T].view(r1 - r0, T)
                if not torch.equal(rr.bit_view(got), rr.bit_view(rows)):
                    bad = (rr.bit_view(got) != rr.bit_view(rows)).nonzero()[:6].cpu().numpy()
                    bad[:, 0] += r0
                    raise AssertionError("%s: rows differ, first at (row, element) %s; lanes %s" %
                                         (rr.run_id(run), bad.tolist(), self.lanes[bad[:, 0] // self.channels].tolist()))
            if table is not None:
                if records is None:
                    records = want_rec[a:b]
                else:
                    records[local] = want_rec[a:b]
                got = table.view[r0 * 4:r1 * 4].view(r1 - r0, 4)
                if not torch.equal(got, records):
                    bad = (got != records).nonzero()[:6].cpu().numpy()
                    bad[:, 0] += r0
                    raise AssertionError("%s: records differ, first at (row, field) %s" % (rr.run_id(run), bad.tolist()))
        if self.rows * T > 1 << 24:
            return None
        return b"".join(bytes(rr.bit_view(f.view).cpu().numpy().tobytes()) for f in (out, table) if f is not None)


def _gains(rng, n):
    g = rng.uniform(-2.0, 2.0, size=n).astype(np.float32)
    g[:4] = [1.0, -1.0, 0.0, 1e-41][:min(n, 4)]
    return g


@pytest.fixture(params=NAMES)
def rig(request, engine):  # noqa: F811
    ratios, wide = rr.resamplers()[request.param]
    r = Rig(engine, ratios, wide)
    yield r
    r.close()


@pytest.fixture(params=NAMES + sorted(rr.SPAN_SETS))
def tile_rig(request, engine):  # noqa: F811
    ratios, wide = dict(rr.resamplers(), **rr.SPAN_SETS)[request.param]
    r = Rig(engine, ratios, wide)
    r.span_set = request.param in rr.SPAN_SETS
    yield r
    r.close()


# ---- a. full tiles behind the first ------------------------------------------------------------------------------------------------------
def test_full_tiles(tile_rig):
    import torch
    rig = tile_rig
    T, C_ = rr.FULL_TILE_FRAMES, 2
    t_src = rig.res.source_frames(T)
    for L, M, _ in rig.banks:
        assert (L, M) in rr.EXEMPT or rr.extra_frame_tiles(L, M, T)
    lanes, window_counts = rr.full_tile_lanes(rig.banks, t_src, T)
    n = len(lanes)
    rng = np.random.default_rng(4097)
    src = _source_rows(rng, n * C_, t_src)
    c_src = np.repeat(window_counts, C_)
    c_src[1::2] = np.roll(window_counts, 1)  # the two rows of a window have counts of their own
    b = Batch(torch, rig, T, C_, lanes, torch.from_numpy(src).cuda(), c_src, rr.spans_for(n, T), _gains(rng, n))
    acc = b.acc.reshape(n, C_, T)
    ended = 0
    for k, (L, M, h) in enumerate(rig.banks):  # the rows that end mid-tile: data in front, zeros once no tap is left on the row
        late, shift = acc[5 * k + 4], int(lanes[5 * k + 4, 1])
        assert (late[:, :2048] != 0).any(axis=1).all()
        silent = [m for m in range(T) if shift + m * M // L - (h.shape[1] // 2 - 1) >= t_src]
        if silent and silent[0] <= 3 * rr.TILE:
            ended += 1
            assert not late[:, silent[0]:].any() and silent[0] > 2 * rr.TILE
    assert ended >= len(rig.banks) // 2
    assert (b.acc[:, 3072:] != 0).any(axis=1).sum() >= b.rows // 2
    if rig.span_set:  # a span one word short for its tile loses the last two taps of a compared output, and the row changes
        assert b.d_src.data_ptr() % 4 == 0
        found = rr.short_span_witnesses(src, lanes, rig.banks, t_src, T, C_)
        assert found
        for name in ("int16", "float32"):
            assert any(ro.convert(b.acc[row, m], name) != ro.convert(b.acc[row, m] - delta, name) for row, m, delta in found), name
    assert (b.counts_full == 0).any() and (b.counts_full == T).any() and ((b.counts_full > 0) & (b.counts_full < T)).any()
    for run in rr.RUNS:
        b.run(run)


# ---- b. source alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", (257, 1025))
def test_source_alignment(rig, frames):
    import torch
    C_ = 2
    needed = rig.res.source_frames(frames)
    lanes = np.array([(bank, shift) for bank, (_, _, h) in enumerate(rig.banks) for shift in (0, h.shape[1] // 2 - 1, h.shape[1] // 2 + 2)],
                     dtype=np.int64)
    n = len(lanes)
    rng = np.random.default_rng(frames)
    src = _source_rows(rng, n * C_, needed)
    c_src = rng.integers(0, needed + 2, size=n * C_)
    spans, gains = rr.spans_for(n, frames), _gains(rng, n)
    written = {}
    for parity in (0, 1):
        for extra in (0, 1):
            pitch = needed + extra
            big = torch.zeros(n * C_ * pitch + parity, dtype=torch.int16, device="cuda")
            d_src = big[parity:].view(n * C_, pitch)
            d_src[:, :needed] = torch.from_numpy(src).cuda()  # the frame past `needed` is a zero: what a shorter row reads there
            assert d_src.data_ptr() % 4 == 2 * parity
            b = Batch(torch, rig, frames, C_, lanes, d_src, c_src, spans, gains, skew=1, front=17)
            assert b.d_gains.data_ptr() % 16 == 4 and b.d_lanes.data_ptr() % 16 == 4 and b.d_spans.data_ptr() % 16 == 8
            assert b.d_source_stats.data_ptr() % 16 == 8
            written[parity, extra] = {rr.run_id(run): b.run(run) for run in rr.RUNS}
    first = written[0, 0]
    assert all(v is not None and len(v) > 0 for v in first.values()) and len(first) == 16
    for key, other in written.items():
        for name, data in other.items():
            assert data == first[name], ("the placement changes the bytes", key, name)


# ---- c. the item loop ------------------------------------------------------------------------------------------------------------------
def test_item_loop(rig):
    import torch
    T, E, G = rr.ITEM_FRAMES, rr.ITEM_EXTRA, rr.GRID
    rows = rr.item_rows()
    kinds, identity = rr.item_kinds(rig.ratios, rig.wide)
    triples = rr.item_triples(kinds)
    t_src = rig.res.source_frames(T)
    rng = np.random.default_rng(2 ** 20 + len(rig.ratios))
    lanes = np.empty((rows, 2), dtype=np.int64)
    lanes[:, 0], lanes[:, 1] = identity, rng.integers(0, 4, size=rows)
    designed = np.concatenate([j * G + np.arange(E) for j in range(3)])
    for j in range(3):  # workgroup b < E takes rows b, 2^20 + b and 2^21 + b
        for b in range(E):
            kind = kinds[triples[b, j]]
            if kind is None:
                lanes[j * G + b] = (ro.NO_BANK, 7)
            else:
                lanes[j * G + b] = (kind, rng.integers(0, rig.banks[kind][2].shape[1] // 2 + 3))
    sample = rng.choice(np.setdiff1d(np.arange(rows), designed), size=4096, replace=False)
    special = np.sort(np.concatenate([designed, sample]))
    d_src = _source_on_device(torch, rows, t_src, seed=77)
    c_src = np.array([0, 2, 5, t_src, t_src + 3], dtype=np.int64)[np.arange(rows) % 5]
    gains = (2.0 ** rng.integers(-3, 3, size=rows) * rng.choice([-1.0, 1.0], size=rows)).astype(np.float32)  # exact in the bulk
    gains[special] = rng.uniform(-2.0, 2.0, size=len(special))
    b = Batch(torch, rig, T, 1, lanes, d_src, c_src, rr.spans_for(rows, T), gains, special=special)
    # before the device is asked: a designed row with a bank is not silent and differs, in int16 and in float32, from the same
    # source row under every other bank of the resampler - a kept or stale bank cannot pass
    at = np.searchsorted(special, designed)
    x, lane = b.src_special[at], b.lanes_special[at]
    under = [rr.expected_acc(x, np.stack([np.full(len(x), k), lane[:, 1]], axis=1), rig.banks, T, 1)[:, 0] for k in range(len(rig.banks))]
    for k in [k for k in kinds if k is not None]:
        mine = lane[:, 0] == k
        assert mine.sum() >= 3 * 8 * len(kinds) ** 2 and np.array_equal(under[k][mine], b.acc[at][mine])
        for name in ("int16", "float32"):
            right = ro.convert(under[k][mine], name)
            assert (right != 0).any(axis=1).all(), (k, name)
            for other in range(len(rig.banks)):
                if other != k:
                    assert (ro.convert(under[other][mine], name) != right).any(axis=1).all(), (k, other, name)
    assert not b.acc[at][lane[:, 0] == ro.NO_BANK].any()
    for run in rr.RUNS:
        b.run(run)


# ---- d. the 2^31 limit -----------------------------------------------------------------------------------------------------------------
LIMIT_RUNS = [("rows", "int16", False), ("rows", "float32", False), ("gain", "float32", False), ("gain", "bfloat16", True),
              ("stats", None, False), ("stats", "float16", False)]


@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("shape", sorted(rr.LIMIT_SHAPES))
def test_index_limit(engine, shape, channels):  # noqa: F811
    import torch
    s = rr.LIMIT_SHAPES[shape]
    T, t_src = s["frames"], s["source_frames"]
    r = Rig(engine, s["ratios"], s["wide"])
    try:
        lib, count = engine.lib, C.c_uint32(9)
        assert lib.AADHip_ResamplerSourceFrames(r.res.handle, T, C.byref(count)) == AADApiResult.OK and count.value == t_src
        assert lib.AADHip_ResamplerSourceFrames(r.res.handle, T + 1, C.byref(count)) == AADApiResult.INVALID_ARGUMENT and count.value == t_src
        lead = r.banks[0][2].shape[1] // 2 - 1
        lanes = np.array([(0, lead), (1, 0), (2, 3), (0, 1)][:4 if channels == 1 else 3], dtype=np.int64)  # every bank, in one launch
        n = len(lanes)
        rng = np.random.default_rng(T)
        src = _source_rows(rng, n * channels, t_src)
        c_src = np.array([t_src, t_src // 2, 0, 5, t_src + 1, 1000][:n * channels], dtype=np.int64)
        spans = np.array([(T - o, o) for o in (1001, 1, 4096, 77777)][:n], dtype=np.int64)  # each ends at the last output
        b = Batch(torch, r, T, channels, lanes, torch.from_numpy(src).cuda(), c_src, spans, _gains(rng, n)[::-1].copy())
        assert (b.acc[:, -rr.TILE:] != 0).any(axis=1).all()  # the last tile of every row has data
        for run in LIMIT_RUNS:
            b.run(run)
    finally:
        r.close()


# ---- e. past 4 GiB ---------------------------------------------------------------------------------------------------------------------
BIG_RUNS = [("rows", "int16", False), ("rows", "float32", False), ("gain", "float32", False), ("stats", "int16", False)]


@pytest.fixture
def big_engine():
    import torch
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ("plain", "wide"))
def test_past_4_gib(big_engine, which):
    import torch
    need = 30  # GiB: the source batch (8.8), float32 rows (16), a chunk's expectation and its index tensors
    free, _ = torch.cuda.mem_get_info()
    if free < (need + 8) * GIB:
        pytest.skip("needs %d GiB of free device memory plus 8 GiB headroom, %.1f GiB free" % (need, free / GIB))
    T, C_, n = rr.BIG_FRAMES, 2, rr.BIG_WINDOWS
    rows = n * C_
    pitch = rr.big_source_frames()
    rig = Rig(big_engine, rr.BIG_WIDE if which == "wide" else rr.BIG_PLAIN, which == "wide")
    d_src = b = None
    try:
        assert rig.res.source_frames(T) == pitch - 1
        witnesses = rr.big_witness_windows()
        rng = np.random.default_rng(4099)
        lanes = np.empty((n, 2), dtype=np.int64)
        lanes[:, 0], lanes[:, 1] = 0, np.arange(n) % 4
        real = list(range(1, len(rig.banks)))
        for k, w in enumerate(witnesses.tolist()):
            bank = real[k % len(real)]
            lanes[w] = (bank, rng.integers(0, rig.banks[bank][2].shape[1] // 2 + 3))
        special = np.sort(np.concatenate([witnesses * 2, witnesses * 2 + 1]))
        d_src = _source_on_device(torch, rows, pitch, seed=4099, parity=1)
        assert d_src.data_ptr() % 4 == 2 and rows * pitch > 1 << 32
        assert bool((d_src[1:, :32] != d_src[:-1, :32]).any(dim=1).all())  # neighbouring rows have different data
        c_src = np.array([0, 2, T // 2, pitch, pitch + 3], dtype=np.int64)[np.arange(rows) % 5]
        gains = (2.0 ** rng.integers(-3, 3, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
        gains[witnesses] = rng.uniform(-2.0, 2.0, size=len(witnesses))
        b = Batch(torch, rig, T, C_, lanes, d_src, c_src, rr.spans_for(n, T), gains, special=special, chunk=1 << 14)
        assert (b.acc != 0).any(axis=1).all()
        for run in BIG_RUNS:
            b.run(run)
            torch.cuda.empty_cache()
    finally:
        rig.close()
        del d_src, b
        torch.cuda.empty_cache()
