"""What aad_amd/engine.py asks of every tensor argument, on the CPU: the engine is made with Engine.__new__ over a library that
records its calls and returns OK, and the tensors are CPU tensors (the device a tensor must be on comes from the engine).

  * run_extent - the elements a run touches from the pointer it is handed - against a plain numpy enumeration of every element
    include/aad_hip.h names for the call, over random small tables; a tensor of exactly that span passes, one element shorter
    is refused, for plain tensors, views that end exactly at the extent and views at a storage offset;
  * one refusal per rule (dtype, device, rank, stride(-1), contiguity, extent, state shape, non-contiguous windows with
    ordered=False, host channel counts, image_size above the row) for every public entry point and every plan run, each with
    no ...Run / ...Batch call reaching the library;
  * one passing call per entry point: the pointers, strides and tables the library received are the tensors' own."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from aad_amd.capi import LANE_STATE_DTYPE, STREAM_DESC_DTYPE, AADHipPlanarLayout, AADHipPlanarOutput, make_parameter
from aad_amd.engine import Engine, run_extent, tensor_span

RUN_CALL = re.compile(r"^AADHip_\w*(PlanRun\w*|Batch)$")
WINDOW_RUNS = ("AADHip_WindowDecodePlanRun", "AADHip_WindowDecodePlanRunStats", "AADHip_WindowReconstructPlanRun")
BLOCK, SPB = 64, 100  # the fake format's block geometry: sizes only have to be consistent


class FakeLib:
    """records (name, args) of every call and returns OK; ...PlanCreate hands out a handle and keeps a copy of the table"""

    def __init__(self):
        self.calls, self.tables = [], {}

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name == "AADHip_CalculateEncodedSize":
                n = int(args[1])
                return 31 + (n + SPB - 1) // SPB * BLOCK if n else 0
            if name == "AADHip_ContextLastError":
                return b""
            if name.endswith("PlanCreate"):
                args[-1]._obj.value = 0x1000 + len(self.calls)
                n, ptr = (args[-4], args[-3]) if "Mix" in name else (args[-3], args[-2])
                raw = C.string_at(ptr, int(n) * STREAM_DESC_DTYPE.itemsize) if n else b""
                self.tables[name] = np.frombuffer(raw, dtype=STREAM_DESC_DTYPE).copy()
            return 0
        return call

    def runs(self):
        return [c for c in self.calls if RUN_CALL.match(c[0])]

    def last(self, name):
        return [c for c in self.calls if c[0] == name][-1][1]


class CpuEngine(Engine):
    """Engine without a device: no streams to order"""

    def _enter(self):
        return None

    def _exit(self, cur):
        pass


@pytest.fixture
def engine():
    e = CpuEngine.__new__(CpuEngine)
    e.torch, e.lib, e.device, e._ctx = torch, FakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def header_bytes(channels, samples, bits=4):
    be = lambda v, n: int(v).to_bytes(n, "big")
    return b"AAD\x00" + be(4, 4) + be(1, 4) + be(channels, 2) + be(samples, 4) + be(48000, 4) + be(bits, 2) + be(BLOCK, 2) + be(SPB, 4) + b"\x00"


def image_tensor(rows, pitch, channels, samples):
    img = torch.zeros((rows, pitch), dtype=torch.uint8)
    img[:, :31] = torch.frombuffer(bytearray(header_bytes(channels, samples)), dtype=torch.uint8)
    return img


# ---- extents against brute force ---------------------------------------------------------------------------------------------

def random_table(rng):
    """1..6 streams in shuffled order with gaps, as a plan's table; C, the strides of a planar layout that holds it, N and T"""
    n = int(rng.integers(1, 7))
    ch = int(rng.choice([1, 2, 3, 8]))
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    d["num_samples"] = rng.integers(1, 12, n)
    d["data_size"] = rng.integers(1, 40, n)
    longest = int(d["num_samples"].max())
    cs = longest + int(rng.integers(0, 4))
    order = rng.permutation(n)
    pos_p = int(rng.integers(0, 5))
    pos_d = int(rng.integers(0, 5))
    for i in order:  # offsets out of order, a gap behind each stream
        d["pcm_offset"][i], d["data_offset"][i] = pos_p, pos_d
        pos_p += max(int(d["num_samples"][i]) * ch, (ch - 1) * cs + int(d["num_samples"][i])) + int(rng.integers(0, 4))
        pos_d += int(d["data_size"][i]) + int(rng.integers(0, 4))
    ss = (ch - 1) * cs + longest + int(rng.integers(0, 4))
    return d, ch, cs, ss, int(rng.integers(1, 5)), int(rng.integers(1, 9))


def brute_force(kind, d, ch, cs, ss, rows, frames):
    """1 + the largest index among the elements include/aad_hip.h names for the kind, enumerated one by one"""
    idx = [-1]
    n = len(d)
    longest = int(d["num_samples"].max())
    for i in range(n):
        po, do, size, ns = (int(d[k][i]) for k in ("pcm_offset", "data_offset", "data_size", "num_samples"))
        if kind == "interleaved":  # P_i[t * C + c] at pcm_offset
            idx += [po + t * ch + c for t in range(ns) for c in range(ch)]
        elif kind == "planar":  # x[pcm_offset + c * channel_stride + t]
            idx += [po + c * cs + t for c in range(ch) for t in range(ns)]
        elif kind == "images":  # [data_offset, data_offset + data_size)
            idx += [do + b for b in range(size)]
        elif kind == "planar_out":  # out[i * stream_stride + c * channel_stride + t]: the layout's row slots, each the longest row long
            idx += [i * ss + c * cs + t for c in range(ch) for t in range(longest)]
    if kind == "window_rows":  # out[(w * C + c) * T + t]
        idx += [(w * ch + c) * frames + t for w in range(rows) for c in range(ch) for t in range(frames)]
    elif kind == "stats":  # record w * C + c, four fields
        idx += [(w * ch + c) * 4 + f for w in range(rows) for c in range(ch) for f in range(4)]
    elif kind == "state":  # record i * C + c, ten int32
        idx += [(i * ch + c) * 10 + f for i in range(rows) for c in range(ch) for f in range(10)]
    return 1 + max(idx)


KINDS = ("interleaved", "planar", "images", "planar_out", "window_rows", "stats", "state")


def test_extents_equal_a_brute_force_enumeration(engine):
    rng = np.random.default_rng(20240)
    for case in range(200):
        d, ch, cs, ss, rows, frames = random_table(rng)
        for kind in KINDS:
            got = run_extent(kind, d, ch, channel_stride=cs, stream_stride=ss, rows=rows, frames=frames)
            want = brute_force(kind, d, ch, cs, ss, rows, frames)
            assert got == want, (case, kind, d.tolist(), ch, cs, ss, rows, frames)
            base = torch.zeros(want + 9, dtype=torch.int16)
            exact = [torch.zeros(want, dtype=torch.int16),        # a tensor of its own
                     base[9:],                                    # a view at a storage offset that ends with the storage
                     base[4:4 + want],                            # a view with storage in front of and behind it
                     torch.zeros((2, want), dtype=torch.int16)[0]]  # a row: the span is the row's, not the storage's
            for t in exact:
                assert tensor_span(t) == want
                engine.tensor("t", t, torch.int16, got, rows_in_place=True)
            for t in (torch.zeros(want - 1, dtype=torch.int16), base[9:-1], base[4:3 + want], torch.zeros((2, want - 1), dtype=torch.int16)[0]):
                with pytest.raises(ValueError, match="t: the run touches %d elements" % want):
                    engine.tensor("t", t, torch.int16, got, rows_in_place=True)
    assert engine.lib.calls == []


def test_span_of_strided_views():
    t = torch.zeros((4, 3, 10))
    assert tensor_span(t) == 120 and tensor_span(t[1:]) == 90 and tensor_span(t[:, :, :7]) == 117
    assert tensor_span(t[::2]) == 60 + 30 and tensor_span(t[:, 1:, 2:5]) == 90 + 10 + 3
    assert tensor_span(t[:0]) == 0 and tensor_span(torch.zeros(())) == 1
    assert tensor_span(torch.zeros(5).expand(3, 5)) == 5
    assert tensor_span(torch.as_strided(torch.zeros(100), (3, 2, 10), (7, 30, 1))) == 1 + 14 + 30 + 9


def test_extents_skip_streams_that_touch_nothing_and_do_not_wrap():
    d = np.zeros(3, dtype=STREAM_DESC_DTYPE)
    d["pcm_offset"], d["data_offset"] = [5, 1 << 40, (1 << 64) - 1], [7, 1 << 40, (1 << 64) - 1]
    d["num_samples"], d["data_size"] = [3, 0, 0], [4, 0, 0]
    assert run_extent("interleaved", d, 2) == 11 and run_extent("planar", d, 2, channel_stride=6) == 14 and run_extent("images", d) == 11
    d["num_samples"][2], d["data_size"][2] = 2, 2
    assert run_extent("interleaved", d, 2) == (1 << 64) + 3 and run_extent("images", d) == (1 << 64) + 1
    assert run_extent("images", d[:0]) == 0 and run_extent("planar_out", d[:0], 2, channel_stride=3, stream_stride=9) == 0


# ---- the plans and tensors of the refusal and pass tests ------------------------------------------------------------------------

N, CH, T = 3, 2, 250          # streams, channels, frames: 2 1/2 blocks of the fake geometry
PARAM = make_parameter(CH, 4, BLOCK)


def ragged_table():
    d = np.zeros(N, dtype=STREAM_DESC_DTYPE)
    d["num_samples"] = [T, 7, 120]
    d["pcm_offset"] = [3, 3 + T * CH + 5, 3 + T * CH + 5 + 7 * CH + 1]
    d["data_size"] = [31 + 3 * BLOCK, 31 + BLOCK, 31 + 2 * BLOCK]
    d["data_offset"] = [64, 0, 64 + 31 + 3 * BLOCK + 9]
    return d


def spoil(t, rule):
    """a tensor that breaks one rule and keeps the others"""
    if rule == "dtype":
        return t.to(torch.float64 if t.dtype != torch.float64 else torch.int8)
    if rule == "device":  # shape, strides and dtype as they were, on a device that is never the engine's
        return torch.empty_like(t, device="meta")
    if rule == "rank":
        return t.reshape((1, 1) + tuple(t.shape)) if t.dim() >= 2 else t.reshape(1, 1, 1, -1)
    if rule == "stride":  # same shape, stride(-1) == 2
        return torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]
    if rule == "noncontiguous":  # same shape, stride(-1) == 1, rows further apart
        return torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), dtype=t.dtype, device=t.device)[..., :t.shape[-1]]
    if rule == "short":  # one element less behind data_ptr()
        return t.reshape(-1)[:-1]
    raise KeyError(rule)


class Call:
    """one entry point or plan run: make(engine) -> (callable(**tensors), dict of good tensors); rules: argument -> rules it must refuse"""

    def __init__(self, name, make, rules):
        self.name, self.make, self.rules = name, make, rules


def _encode_plan_run(e):
    d = ragged_table()
    plan = e.encode_plan(PARAM, d)
    good = dict(pcm=torch.zeros(run_extent("interleaved", d, CH), dtype=torch.int16), data=torch.zeros(run_extent("images", d), dtype=torch.uint8),
                state=torch.zeros((N * CH, 10), dtype=torch.int32))
    return (lambda pcm, data, state: plan.run(pcm, data, state)), good


def _decode_plan_run(e):
    d = ragged_table()
    plan = e.decode_plan(_header(), d)
    good = dict(data=torch.zeros(run_extent("images", d), dtype=torch.uint8), pcm=torch.zeros(run_extent("interleaved", d, CH), dtype=torch.int16))
    return (lambda data, pcm: plan.run(data, pcm)), good


def _header(channels=CH, samples=T):
    from aad_amd.engine import parse_header
    return parse_header(header_bytes(channels, samples))


CS, OSS, OCS = T + 3, CH * (T + 2) + 5, T + 2   # input channel stride; output stream and channel strides


def _planar_table():
    d = ragged_table()
    d["pcm_offset"] = [2, 2 + CH * CS + 1, 2 + 2 * CH * CS + 7]
    return d


def _planar_encode_plan_run(e):
    d = _planar_table()
    plan = e.planar_encode_plan(PARAM, d, CS, torch.float32)
    good = dict(x=torch.zeros(run_extent("planar", d, CH, channel_stride=CS)), data=torch.zeros(run_extent("images", d), dtype=torch.uint8),
                state=torch.zeros((N * CH, 10), dtype=torch.int32))
    return (lambda x, data, state: plan.run(x, data, state)), good


def _planar_reconstruct_plan_run(e):
    d = _planar_table()
    plan = e.planar_reconstruct_plan(PARAM, d, CS, torch.int16, torch.float32, OSS, OCS)
    good = dict(x=torch.zeros(run_extent("planar", d, CH, channel_stride=CS), dtype=torch.int16),
                data=torch.zeros(run_extent("images", d), dtype=torch.uint8),
                out=torch.zeros(run_extent("planar_out", d, CH, channel_stride=OCS, stream_stride=OSS)),
                state=torch.zeros((N * CH, 10), dtype=torch.int32), stats=torch.zeros((N, CH, 4), dtype=torch.int64))
    return (lambda x, data, out, state, stats: plan.run(x, data, out, state, stats=stats)), good


W, FRAMES = 4, 17  # windows of a window run


def _window_decode_plan_run(e, ordered=True):
    d = ragged_table()
    plan = e.window_decode_plan(_header(), d)
    good = dict(data=torch.zeros(run_extent("images", d), dtype=torch.uint8), windows=torch.zeros((W, 2), dtype=torch.int64),
                out=torch.zeros((W, CH, FRAMES)), stats=torch.zeros((W, CH, 4), dtype=torch.int64))
    return (lambda data, windows, out, stats: plan.run(data, windows, FRAMES, out=out, stats=stats, ordered=ordered)), good


def _window_reconstruct_plan_run(e, ordered=True):
    d = _planar_table()
    plan = e.window_reconstruct_plan(PARAM, d, CS, torch.int16)
    good = dict(x=torch.zeros(run_extent("planar", d, CH, channel_stride=CS), dtype=torch.int16), windows=torch.zeros((W, 2), dtype=torch.int64),
                out=torch.zeros((W, CH, FRAMES)), data=torch.zeros((W, 31 + BLOCK), dtype=torch.uint8),
                stats=torch.zeros((W, CH, 4), dtype=torch.int64))
    return (lambda x, windows, out, data, stats: plan.run(x, windows, FRAMES, out=out, data=data, stats=stats, ordered=ordered)), good


def _uniform(fn):
    def make(e):
        good = dict(pcm=torch.zeros((N, T, CH), dtype=torch.int16))
        if fn == "encode_uniform":
            good["state"] = torch.zeros((N * CH, 10), dtype=torch.int32)
            return (lambda pcm, state: e.encode_uniform(pcm, PARAM, state)), good
        return (lambda pcm: e.reconstruct_uniform(pcm, PARAM)), good
    return make


def _planar(fn):
    def make(e):
        good = dict(x=torch.zeros((N, CH, T)))
        if fn == "encode_planar_mixed":
            return (lambda x: e.encode_planar_mixed(x, lambda b: make_parameter(CH, b, BLOCK), [2, 3, 4])), good
        good["state"] = torch.zeros((N * CH, 10), dtype=torch.int32)
        return (lambda x, state: getattr(e, fn)(x, PARAM, state=state)), good
    return make


def _windows_of_corpus(fn):
    def make(e):
        good = dict(corpus=torch.zeros((N, CH, T), dtype=torch.int16), windows=torch.zeros((W, 2), dtype=torch.int64))
        return (lambda corpus, windows: getattr(e, fn)(corpus, windows, FRAMES, PARAM)), good
    return make


PITCH, SIZE = 31 + 3 * BLOCK + 33, 31 + 3 * BLOCK  # the rows of an image tensor and the images in them


def _images(fn):
    def make(e):
        good = dict(data=image_tensor(N, PITCH, CH, T))
        if fn == "decode_uniform":
            return (lambda data: e.decode_uniform(data, SIZE)), good
        good["windows"] = torch.zeros((W, 2), dtype=torch.int64)
        if fn == "window_levels":
            return (lambda data, windows: e.window_levels(data, SIZE, windows, FRAMES)), good
        return (lambda data, windows: getattr(e, fn)(data, SIZE, windows, FRAMES)), good
    return make


ROWS = ("dtype", "device", "stride", "short")          # a flat buffer behind a table
STATE = ("dtype", "device", "rank", "stride", "short")  # [lanes, 10]: short is a wrong shape, stride a non-contiguous table
TABLE = ("dtype", "device", "rank", "stride", "noncontiguous", "short")  # contiguous tensors of one shape
VIEW3 = ("dtype", "device", "rank", "stride")           # [N, C, T] views read in place: their own span is what is read
CALLS = [
    Call("EncodePlan.run", _encode_plan_run, dict(pcm=ROWS, data=ROWS, state=STATE)),
    Call("DecodePlan.run", _decode_plan_run, dict(data=ROWS, pcm=ROWS)),
    Call("PlanarEncodePlan.run", _planar_encode_plan_run, dict(x=ROWS, data=ROWS, state=STATE)),
    Call("PlanarReconstructPlan.run", _planar_reconstruct_plan_run, dict(x=ROWS, data=ROWS, out=ROWS, state=STATE, stats=TABLE)),
    Call("WindowDecodePlan.run", _window_decode_plan_run, dict(data=ROWS, windows=("dtype", "device", "rank", "short"), out=TABLE, stats=TABLE)),
    Call("WindowReconstructPlan.run", _window_reconstruct_plan_run,
         dict(x=ROWS, windows=("dtype", "device", "rank", "short"), out=VIEW3 + ("short",), data=("dtype", "device", "rank", "stride", "short"), stats=TABLE)),
    Call("encode_uniform", _uniform("encode_uniform"), dict(pcm=("dtype", "device", "rank", "stride", "noncontiguous"), state=STATE)),
    Call("reconstruct_uniform", _uniform("reconstruct_uniform"), dict(pcm=("dtype", "device", "rank", "stride", "noncontiguous"))),
    Call("encode_planar", _planar("encode_planar"), dict(x=VIEW3, state=STATE)),
    Call("encode_planar_mixed", _planar("encode_planar_mixed"), dict(x=VIEW3)),
    Call("reconstruct_planar", _planar("reconstruct_planar"), dict(x=VIEW3, state=STATE)),
    Call("codec_error", _planar("codec_error"), dict(x=VIEW3, state=STATE)),
    Call("reconstruct_windows", _windows_of_corpus("reconstruct_windows"), dict(corpus=VIEW3, windows=("dtype", "device", "rank", "short"))),
    Call("codec_error_windows", _windows_of_corpus("codec_error_windows"), dict(corpus=VIEW3, windows=("dtype", "device", "rank", "short"))),
    Call("decode_uniform", _images("decode_uniform"), dict(data=VIEW3)),
    Call("decode_windows", _images("decode_windows"), dict(data=VIEW3, windows=("dtype", "device", "rank", "short"))),
    Call("decode_windows_mixed", _images("decode_windows_mixed"), dict(data=VIEW3, windows=("dtype", "device", "rank", "short"))),
    Call("window_levels", _images("window_levels"), dict(data=VIEW3, windows=("dtype", "device", "rank", "short"))),
]
REFUSALS = [(c, arg, rule) for c in CALLS for arg, rules in c.rules.items() for rule in rules]


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c.name)
def test_the_good_call_passes(engine, call):
    """the tensors the refusals start from are accepted: every refusal below is the one spoiled rule's"""
    fn, good = call.make(engine)
    fn(**good)
    assert len(engine.lib.runs()) >= 1


@pytest.mark.parametrize("call,arg,rule", REFUSALS, ids=lambda v: v.name if isinstance(v, Call) else v)
def test_one_broken_rule_is_refused_before_any_run(engine, call, arg, rule):
    fn, good = call.make(engine)
    bad = dict(good)
    bad[arg] = spoil(good[arg], rule)
    with pytest.raises(ValueError, match=r"\b%s\b" % arg):
        fn(**bad)
    assert engine.lib.runs() == []


def test_a_second_run_with_another_layout_is_checked_again(engine):
    """a plan remembers the layout that passed; a different one does not ride on it"""
    fn, good = _encode_plan_run(engine)
    fn(**good)
    fn(**good)
    assert len(engine.lib.runs()) == 2
    for arg in ("pcm", "data"):
        with pytest.raises(ValueError, match=arg):
            fn(**dict(good, **{arg: spoil(good[arg], "short")}))
    with pytest.raises(ValueError, match="state"):
        fn(**dict(good, state=torch.zeros((N * CH, 9), dtype=torch.int32)))
    assert len(engine.lib.runs()) == 2


@pytest.mark.parametrize("make", [_window_decode_plan_run, _window_reconstruct_plan_run], ids=["WindowDecodePlan", "WindowReconstructPlan"])
def test_non_contiguous_windows_need_an_ordered_run(engine, make):
    views = [torch.zeros((W, 3), dtype=torch.int64)[:, :2], torch.zeros((2, W), dtype=torch.int64).t()]
    fn, good = make(engine, ordered=False)
    for w in views:
        with pytest.raises(ValueError, match="windows: a contiguous tensor is needed with ordered=False"):
            fn(**dict(good, windows=w))
    assert engine.lib.runs() == []
    fn(**good)  # a contiguous table is fine unordered
    fn, good = make(engine, ordered=True)
    for w in views:  # ordered: the copy is handed over, not the view
        fn(**dict(good, windows=w))
        name, args = engine.lib.runs()[-1]
        assert name in WINDOW_RUNS and args[3] != w.data_ptr()
    fn(**good)
    assert engine.lib.runs()[-1][1][3] == good["windows"].data_ptr()


def test_planar_rows_that_overlap_are_refused(engine):
    mono = torch.zeros((N, 1, T), dtype=torch.int16)
    for call in (lambda x: engine.encode_planar(x, PARAM), lambda x: engine.reconstruct_planar(x, PARAM), lambda x: engine.codec_error(x, PARAM),
                 lambda x: engine.encode_planar_mixed(x, lambda b: make_parameter(CH, b, BLOCK), [4] * N),
                 lambda x: engine.reconstruct_windows(x, torch.zeros((W, 2), dtype=torch.int64), FRAMES, PARAM)):
        with pytest.raises(ValueError, match=r"channel stride 0 \(stride\(1\)\)"):
            call(mono.expand(N, 2, T))
    x = torch.as_strided(torch.zeros(4 * T), (N, CH, T), (T // 2, T + 1, 1))  # streams overlap each other: the input is only read
    engine.encode_planar(x, PARAM)
    assert len(engine.lib.runs()) == 1 and engine.lib.calls[-2][0] == "AADHip_PlanarEncodePlanRun"


def test_image_sizes_above_the_row_are_refused(engine):
    img = image_tensor(N, PITCH, CH, T)
    win = torch.zeros((W, 2), dtype=torch.int64)
    for data in (img, img[:, :SIZE], img[:1]):
        width = data.shape[1]
        for call in (lambda: engine.decode_uniform(data, width + 1), lambda: engine.decode_windows(data, width + 1, win, FRAMES),
                     lambda: engine.decode_windows_mixed(data, [width] * (len(data) - 1) + [width + 1], win, FRAMES),
                     lambda: engine.window_levels(data, width + 1, win, FRAMES)):
            with pytest.raises(ValueError, match="data: an image of %d bytes is needed in every row, the rows have %d" % (width + 1, width)):
                call()
    with pytest.raises(ValueError, match="data: at least one image"):
        engine.decode_uniform(img[:0], SIZE)
    assert engine.lib.runs() == [] and not any(n.endswith("PlanCreate") for n, _ in engine.lib.calls)


def test_host_arrays_must_have_the_parameters_channels(engine):
    stereo, mono = make_parameter(2, 4, BLOCK), make_parameter(1, 4, BLOCK)
    for call in (engine.encode_host, engine.reconstruct_host):
        for bad in ([np.zeros((50, 1), dtype=np.int16)], [np.zeros((50, 2), dtype=np.int16), np.zeros(50, dtype=np.int16)],
                    [np.zeros((50, 3), dtype=np.int16)], [np.zeros((2, 50, 2), dtype=np.int16)]):
            with pytest.raises(ValueError, match=r"pcm_list\[%d\]: an array \[samples, 2\]" % (len(bad) - 1)):
                call(bad, stereo)
        with pytest.raises(ValueError, match=r"pcm_list\[0\]"):
            call([np.zeros((50, 2), dtype=np.int16)], mono)
    assert engine.lib.runs() == []
    engine.encode_host([np.zeros(50, dtype=np.int16), np.zeros((20, 1), dtype=np.int16)], mono)  # mono: 1-D or [n, 1]
    engine.reconstruct_host([np.zeros(50, dtype=np.int16), np.zeros((20, 1), dtype=np.int16)], mono)
    assert [n for n, _ in engine.lib.runs()] == ["AADHip_EncodeBatch", "AADHip_ReconstructBatch"]


def test_encode_host_state_must_be_the_batchs_records(engine):
    pcms = [np.zeros((50, 2), dtype=np.int16)] * 3
    for bad in (np.zeros(6, dtype=[("w", "<i4", 10)]), np.zeros((6, 10), dtype=np.int32), np.zeros(5, dtype=LANE_STATE_DTYPE),
                np.zeros(7, dtype=LANE_STATE_DTYPE), np.zeros(12, dtype=LANE_STATE_DTYPE)[::2], torch.zeros((6, 10), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"state: a contiguous LANE_STATE_DTYPE array \[6\]"):
            engine.encode_host(pcms, PARAM, state=bad)
    assert engine.lib.runs() == []
    state = np.zeros(6, dtype=LANE_STATE_DTYPE)
    engine.encode_host(pcms, PARAM, state=state)
    assert engine.lib.last("AADHip_EncodeBatch")[-1] == state.ctypes.data


# ---- what the library is handed ------------------------------------------------------------------------------------------------

def test_plan_runs_hand_over_the_tensors_own_pointers(engine):
    for make, name, order in ((_encode_plan_run, "AADHip_EncodePlanRun", ("pcm", "data", "state")),
                              (_decode_plan_run, "AADHip_DecodePlanRun", ("data", "pcm")),
                              (_planar_encode_plan_run, "AADHip_PlanarEncodePlanRun", ("x", "data", "state")),
                              (_planar_reconstruct_plan_run, "AADHip_PlanarReconstructPlanRunStats", ("x", "data", "out", "state", "stats"))):
        fn, good = make(engine)
        base = {k: torch.zeros(v.numel() + 5, dtype=v.dtype) for k, v in good.items()}
        views = {k: base[k][5:].view(v.shape) for k, v in good.items()}  # every argument at a storage offset
        fn(**views)
        args = engine.lib.last(name)
        assert list(args[1:]) == [views[k].data_ptr() for k in order], name
        assert all(views[k].data_ptr() == base[k].data_ptr() + 5 * base[k].element_size() for k in order)


def test_window_runs_hand_over_pointers_strides_and_counts(engine):
    fn, good = _window_decode_plan_run(engine)
    fn(**good)
    args = engine.lib.last("AADHip_WindowDecodePlanRunStats")
    assert list(args[1:]) == [good["data"].data_ptr(), W, good["windows"].data_ptr(), FRAMES, 1, good["out"].data_ptr(), good["stats"].data_ptr()]
    fn, good = _window_reconstruct_plan_run(engine)
    out = torch.zeros((W + 1, CH + 1, FRAMES + 3))[1:, 1:, 2:2 + FRAMES]      # rows written in place: its strides go to the library
    data = torch.zeros((W, 31 + BLOCK + 40), dtype=torch.uint8)[:, 7:38 + BLOCK]
    fn(**dict(good, out=out, data=data))
    args = engine.lib.last("AADHip_WindowReconstructPlanRun")
    assert (args[1], args[2], args[3], args[4]) == (good["x"].data_ptr(), W, good["windows"].data_ptr(), FRAMES)
    assert (args[5], args[6]) == (data.stride(0), data.data_ptr()) and args[8] == out.data_ptr() and args[9] == good["stats"].data_ptr()
    output = args[7]._obj
    assert (output.stream_stride, output.channel_stride, output.sample_type) == (out.stride(0), out.stride(1), 1)


@pytest.mark.parametrize("fn", ["encode_planar", "reconstruct_planar", "codec_error", "encode_planar_mixed", "reconstruct_windows"])
def test_planar_views_are_read_where_they_lie(engine, fn):
    big = torch.zeros((2 * N + 1, CH + 1, T + 9), dtype=torch.int16)
    x = big[1::2, 1:, 4:4 + T]  # every other stream, a channel skipped, rows at an odd offset
    assert not x.is_contiguous() and x.stride(-1) == 1
    win = torch.zeros((W, 2), dtype=torch.int64)
    if fn == "encode_planar_mixed":
        engine.encode_planar_mixed(x, lambda b: make_parameter(CH, b, BLOCK), [4] * N)
    elif fn == "reconstruct_windows":
        engine.reconstruct_windows(x, win, FRAMES, PARAM)
    else:
        getattr(engine, fn)(x, PARAM)
    create = [n for n, _ in engine.lib.calls if n.endswith("PlanCreate")][0]
    layout = [a._obj for a in engine.lib.last(create) if hasattr(a, "_obj") and isinstance(a._obj, AADHipPlanarLayout)][0]
    assert layout.channel_stride == x.stride(1)
    assert engine.lib.tables[create]["pcm_offset"].tolist() == [i * x.stride(0) for i in range(N)]
    name, args = engine.lib.runs()[0]
    assert args[1] == x.data_ptr() == big.data_ptr() + 2 * big[1, 1, 4:].storage_offset()
    if fn == "reconstruct_planar":
        out = [a._obj for a in engine.lib.last(create) if hasattr(a, "_obj") and isinstance(a._obj, AADHipPlanarOutput)][0]
        assert (out.stream_stride, out.channel_stride) == (CH * T, T)


def test_uniform_entry_points_hand_over_the_contiguous_tensor(engine):
    pcm = torch.zeros((N + 1, T, CH), dtype=torch.int16)[1:]  # contiguous at a storage offset
    state = torch.zeros((N * CH, 10), dtype=torch.int32)
    out, size = engine.encode_uniform(pcm, PARAM, state)
    args = engine.lib.last("AADHip_EncodePlanRun")
    assert list(args[1:]) == [pcm.data_ptr(), out.data_ptr(), state.data_ptr()] and size == 31 + 3 * BLOCK
    table = engine.lib.tables["AADHip_EncodePlanCreate"]
    assert table["pcm_offset"].tolist() == [i * T * CH for i in range(N)] and table["data_offset"].tolist() == [i * out.stride(0) for i in range(N)]
    rec, stats = engine.reconstruct_uniform(pcm, PARAM)
    args = engine.lib.last("AADHip_ReconstructPlanRun")
    assert args[1] == pcm.data_ptr() and args[3] == rec.data_ptr() and args[5] == stats.data_ptr() and rec.is_contiguous()


VIEWS = {"columns": lambda img: img[:, :SIZE], "every_other_row": lambda img: img[::2], "contiguous": lambda img: img}


@pytest.mark.parametrize("view", list(VIEWS))
def test_decode_uniform_takes_the_row_pitch_from_the_stride(engine, view):
    """decode_uniform(img[:, :size]) and decode_uniform(img[::2]): stream i's image lies at i * data.stride(0).
    FAILS ON THE PARENT COMMIT for "columns" and "every_other_row": its table used data.shape[1] as the pitch, so every
    stream but the first was decoded from another row's bytes."""
    data = VIEWS[view](image_tensor(2 * N, PITCH, CH, T))
    pcm, header = engine.decode_uniform(data, SIZE)
    table = engine.lib.tables["AADHip_DecodePlanCreate"]
    assert table["data_offset"].tolist() == [i * data.stride(0) for i in range(len(data))]
    assert table["data_size"].tolist() == [SIZE] * len(data) and table["num_samples"].tolist() == [T] * len(data)
    args = engine.lib.last("AADHip_DecodePlanRun")
    assert args[1] == data.data_ptr() and args[2] == pcm.data_ptr() and tuple(pcm.shape) == (len(data), T, CH)


@pytest.mark.parametrize("view", list(VIEWS))
def test_decode_windows_takes_the_row_pitch_from_the_stride(engine, view):
    """decode_windows(img[:, :size], ...) and decode_windows(img[::2], ...): as decode_uniform.  FAILS ON THE PARENT COMMIT for
    "columns" and "every_other_row": the table it handed to AADHip_WindowDecodePlanCreate had data.shape[1] as the pitch,
    [0, 223, 446, ...] for the strided [0, 256, 512, ...] (the parent also refuses every CPU window table, so there the test stops
    at that refusal, with the wrong table already made).  decode_windows_mixed and window_levels always took data.stride(0) and
    are held to the same table here."""
    data = VIEWS[view](image_tensor(2 * N, PITCH, CH, T))
    win = torch.zeros((W, 2), dtype=torch.int64)
    want = [i * data.stride(0) for i in range(len(data))]
    rows = engine.decode_windows(data, SIZE, win, FRAMES, torch.int16)
    assert engine.lib.tables["AADHip_WindowDecodePlanCreate"]["data_offset"].tolist() == want
    args = engine.lib.last("AADHip_WindowDecodePlanRun")
    assert (args[1], args[2], args[3], args[4], args[5], args[6]) == (data.data_ptr(), W, win.data_ptr(), FRAMES, 0, rows.data_ptr())
    engine.decode_windows_mixed(data, SIZE, win, FRAMES)
    assert engine.lib.tables["AADHip_MixedWindowDecodePlanCreate"]["data_offset"].tolist() == want
    engine.window_levels(data, SIZE, win, FRAMES, channels=2)
    assert engine.lib.tables["AADHip_ChannelMixWindowDecodePlanCreate"]["data_offset"].tolist() == want
    assert engine.lib.last("AADHip_WindowDecodePlanRunStats")[1] == data.data_ptr()
