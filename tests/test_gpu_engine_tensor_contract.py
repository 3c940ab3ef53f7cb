"""aad_amd/engine.py's tensor contract on the device: every tensor argument of every entry point and plan run handed over as a
view - at a storage offset that puts int16 rows on odd 2-byte alignments, with a row pitch wider than the row, row-sliced,
overlapping - laid inside a larger buffer of canaries.  The result must equal the all-contiguous call's and the oracle's
(tests/oracle_binding.py, tests/window_oracle.py, tests/window_stats_oracle.py) bit for bit, and every canary around every
written tensor must survive.  No tolerances anywhere.

Shapes: 5 streams, max_block_size 128, 2 1/2 blocks of frames, 4 and 2 bits, mono and stereo, windows of 1, 17 and spb + 3 frames.

Refusals run on an engine whose library raises AssertionError from every ...Run... / ...Batch entry: a missing check fails the
test instead of launching.  Nothing here reaches a launch with a bad pointer; an over-READ past an extent cannot be observed
without faulting and is covered by tests/test_engine_tensor_contract.py and the contract in include/aad_hip.h alone."""
import functools
import re

import numpy as np
import pytest

import oracle_binding as ob
from aad_amd.capi import STREAM_DESC_DTYPE, make_parameter
from aad_amd.engine import parse_header, run_extent
from aad_amd.synth import synth_pcm
from window_oracle import window_expected
from window_stats_oracle import window_stats_expected

pytestmark = pytest.mark.gpu

MBS, STREAMS = 128, 5
CASES = [(1, 4), (2, 4), (1, 2), (2, 2)]  # (channels, bits)
CASE_IDS = ["%dch%db" % c for c in CASES]
CANARIES = {"int16": 0x5A5A, "uint8": 0x5A, "float32": 0x7FA5A5A5, "int64": 0x5A5A5A5A5A5A5A5A, "int32": 0x5A5A5A5A}


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


class RefusingLibrary:
    """the real library, but for its run entries: reaching one with an argument that should have been refused fails the test"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if re.match(r"^AADHip_\w*(Run\w*|Batch)$", name):
            raise AssertionError("%s was reached: a refusal is missing" % name)
        return getattr(self._lib, name)


@pytest.fixture(scope="module")
def refusing(engine):
    from aad_amd.engine import Engine
    e = Engine(0, lib=RefusingLibrary(engine.lib))
    yield e
    e.close()


# ---- views inside canaries ------------------------------------------------------------------------------------------------------

def _bits_dtype(torch, dtype):
    return {torch.float32: torch.int32}.get(dtype, dtype)


def _name(dtype):
    return str(dtype).split(".")[-1]


def canary_buffer(torch, count, dtype, device):
    """`count` elements of dtype, every one the dtype's canary (float32: a NaN with a payload)"""
    return torch.full((count,), CANARIES[_name(dtype)], dtype=_bits_dtype(torch, dtype), device=device).view(dtype)


def laid(torch, t, strides, lead, tail=11):
    """-> (buffer, view): a view equal to `t` with the given strides at storage offset `lead` of a buffer of canaries"""
    span = 1 + sum((s - 1) * st for s, st in zip(t.shape, strides)) if t.numel() else 0
    buffer = canary_buffer(torch, lead + span + tail, t.dtype, t.device)
    view = torch.as_strided(buffer, tuple(t.shape), tuple(strides), lead)
    view.copy_(t)
    return buffer, view


def embedded(torch, t, lead, pad):
    """-> (buffer, view): a view equal to `t` inside a larger buffer filled with the dtype's canary, at the non-zero storage offset
    `lead` (odd: int16 rows land on odd 2-byte alignments) and with a row pitch `pad` elements wider than the row"""
    pitch = int(t.shape[-1]) + pad
    strides, step = [1], pitch
    for s in reversed(t.shape[1:-1] if t.dim() > 1 else ()):
        strides.insert(0, step)
        step *= int(s)
    if t.dim() > 1:
        strides.insert(0, step)
    return laid(torch, t, strides, lead, tail=pad + 11)


def untouched(torch, buffer, view, label=""):
    """every canary element of `buffer` outside `view` still holds the canary"""
    outside = torch.ones(buffer.numel(), dtype=torch.bool, device=buffer.device)
    torch.as_strided(outside, tuple(view.shape), tuple(view.stride()), view.storage_offset() - buffer.storage_offset()).fill_(False)
    bits = buffer.view(_bits_dtype(torch, buffer.dtype))
    bad = torch.nonzero(outside & (bits != CANARIES[_name(buffer.dtype)]))
    assert bad.numel() == 0, (label, "a canary outside the view was overwritten, first at element", int(bad[0]), "view offset",
                              view.storage_offset(), "shape", tuple(view.shape), "strides", tuple(view.stride()))


def test_embedded_views_and_their_canaries():
    import torch
    t = torch.arange(5 * 2 * 9, dtype=torch.int16, device="cuda").view(5, 2, 9)
    buffer, view = embedded(torch, t, 3, 4)
    assert torch.equal(view, t) and view.storage_offset() == 3 and tuple(view.stride()) == (26, 13, 1) and view.data_ptr() % 4 == 2
    untouched(torch, buffer, view)
    for spot in (0, 2, 3 + 9, buffer.numel() - 1):  # in front, the last lead element, the first pad element, the end
        b2 = buffer.clone()
        b2[spot] = 1
        with pytest.raises(AssertionError):
            untouched(torch, b2, torch.as_strided(b2, (5, 2, 9), (26, 13, 1), 3))
    f = torch.linspace(-1, 1, 12, device="cuda").view(3, 4)
    buffer, view = embedded(torch, f, 1, 2)
    assert torch.equal(view, f) and bool(torch.isnan(buffer[0])) and buffer.view(torch.int32)[0].item() == 0x7FA5A5A5
    untouched(torch, buffer, view)
    flat, v1 = embedded(torch, torch.zeros(10, dtype=torch.uint8, device="cuda"), 5, 0)
    assert v1.is_contiguous() and v1.storage_offset() == 5 and flat[4].item() == 0x5A and flat[15].item() == 0x5A


# ---- the corpus: oracle images of synthetic streams ------------------------------------------------------------------------------

def round64(v):
    return -(-int(v) // 64) * 64


@functools.lru_cache(maxsize=None)
def corpus(ch, bits):
    rc, block, spb = ob.geometry(MBS, ch, bits)
    assert rc == 0
    n = 2 * spb + spb // 2
    pcm = synth_pcm(2 * STREAMS, n, ch, seed=4100 + 10 * ch + bits)
    images = [ob.encode(pcm[s], bits, MBS) for s in range(2 * STREAMS)]
    decoded = [ob.decode(img)[0] for img in images]
    assert len({len(i) for i in images}) == 1
    return dict(ch=ch, bits=bits, spb=spb, n=n, pcm=pcm, images=images, decoded=decoded, size=len(images[0]),
                param=make_parameter(ch, bits, MBS, 48000, False, 0))


def image_rows(torch, c):
    """uint8 [10, pitch]: row s starts with stream s's image, the bytes behind it are not zeros"""
    pitch = round64(c["size"]) + 64
    host = np.full((2 * STREAMS, pitch), 0xC3, dtype=np.uint8)
    for s, img in enumerate(c["images"]):
        host[s, :c["size"]] = np.frombuffer(img, dtype=np.uint8)
    return torch.from_numpy(host).cuda()


def windows_for(n_streams, n, spb, frames):
    rows = [(0, 0), (1 % n_streams, spb), (n_streams - 1, spb - 1), (2 % n_streams, spb + 5), (n_streams - 1, 2 * spb - 3),
            (0, max(n - frames, 0)), (1 % n_streams, n - 1), (3 % n_streams, n), (n_streams, 0), (-1, 3), (2 % n_streams, -1)]
    return np.array(rows, dtype=np.int64)


def data_views(torch, img, size):
    """(label, the streams the view shows, buffer or None, view) for img[:, :size] and img[::2], plain and embedded"""
    out = []
    for label, view, streams in (("img[:, :size]", img[:, :size], list(range(2 * STREAMS))), ("img[::2]", img[::2], list(range(0, 2 * STREAMS, 2)))):
        assert not view.is_contiguous() and view.stride(1) == 1
        out.append((label, streams, None, view))
        buffer, inside = embedded(torch, view, 3, 5)
        out.append((label + " embedded", streams, buffer, inside))
    return out


# ---- uniform decode paths over row-sliced and column-sliced data ----------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_uniform_decode_paths_read_views_in_place(engine, case):
    import torch
    c = corpus(*case)
    ch, n, spb, size = c["ch"], c["n"], c["spb"], c["size"]
    img = image_rows(torch, c)
    for label, streams, buffer, data in data_views(torch, img, size):
        decoded = [c["decoded"][s] for s in streams]
        plain = data.contiguous()
        pcm, header = engine.decode_uniform(data, size)
        assert header.num_samples == n and np.array_equal(pcm.cpu().numpy(), np.stack(decoded)), (label, "decode_uniform")
        assert torch.equal(pcm, engine.decode_uniform(plain, size)[0]), (label, "decode_uniform against the contiguous call")
        for frames in (1, 17, spb + 3):
            win = windows_for(len(streams), n, spb, frames)
            d_win = torch.from_numpy(win).cuda()
            want16 = window_expected(decoded, win, frames, ch)
            want32 = want16.astype(np.float32) / np.float32(32768.0)
            want_stats = window_stats_expected(decoded, win, frames, ch)
            got16 = engine.decode_windows(data, size, d_win, frames, torch.int16)
            assert np.array_equal(got16.cpu().numpy(), want16), (label, frames, "decode_windows int16")
            assert torch.equal(got16, engine.decode_windows(plain, size, d_win, frames, torch.int16)), (label, frames, "against the contiguous call")
            wbuf, wview = embedded(torch, d_win, 1, 1)  # the window table as a view: [N, 2] rows three apart
            assert not wview.is_contiguous()
            assert torch.equal(engine.decode_windows(plain, size, wview, frames, torch.int16), got16), (label, frames, "windows as a view")
            untouched(torch, wbuf, wview, "windows")
            got32 = engine.decode_windows(data, size, d_win, frames)
            assert np.array_equal(got32.cpu().numpy().view(np.uint32), want32.view(np.uint32)), (label, frames, "decode_windows float32")
            got_half = engine.decode_windows(data, size, d_win, frames, torch.float16)
            assert torch.equal(got_half.cpu().view(torch.int16), torch.from_numpy(want32).to(torch.float16).view(torch.int16)), (label, frames, "float16")
            rows, stats = engine.decode_windows(data, size, d_win, frames, torch.int16, return_stats=True)
            assert np.array_equal(rows.cpu().numpy(), want16) and np.array_equal(stats.cpu().numpy(), want_stats), (label, frames, "return_stats")
            mixed, mstats = engine.decode_windows_mixed(data, size, d_win, frames, torch.int16, return_stats=True)
            assert np.array_equal(mixed.cpu().numpy(), want16) and np.array_equal(mstats.cpu().numpy(), want_stats), (label, frames, "mixed")
            levels = engine.window_levels(data, [size] * len(streams), d_win, frames)
            assert np.array_equal(levels.cpu().numpy(), want_stats), (label, frames, "window_levels")
        if buffer is not None:
            untouched(torch, buffer, data, label)


@pytest.mark.parametrize("case", [(2, 4), (1, 2)], ids=["2ch4b", "1ch2b"])
def test_window_decode_run_takes_views_of_a_window_table(engine, case):
    """windows as table3[:, :2] and as t2.t(): ordered=True copies them, and the copy outlives the kernel's read of it - on the
    default stream, and on a non-default torch stream where a tensor of the same size is asked for right behind the call and
    filled with windows that decode to zeros"""
    import torch
    c = corpus(*case)
    ch, n, spb, size = c["ch"], c["n"], c["spb"], c["size"]
    img = image_rows(torch, c)
    plan = engine.uniform_window_decode_plan(parse_header(c["images"][0][:31]), 2 * STREAMS, img.stride(0), size)
    try:
        for frames in (1, 17, spb + 3):
            win = windows_for(2 * STREAMS, n, spb, frames)
            want = window_expected(c["decoded"], win, frames, ch)
            table3 = torch.full((len(win), 3), CANARIES["int64"], dtype=torch.int64, device="cuda")
            table3[:, :2] = torch.from_numpy(win).cuda()
            t2 = torch.from_numpy(np.ascontiguousarray(win.T)).cuda()
            for label, view in (("table3[:, :2]", table3[:, :2]), ("t2.t()", t2.t())):
                assert not view.is_contiguous()
                got = plan.run(img, view, frames, torch.int16)
                assert np.array_equal(got.cpu().numpy(), want), (label, frames, "default stream")
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    got = plan.run(img, view, frames, torch.int16)
                    reuse = torch.empty((len(win), 2), dtype=torch.int64, device="cuda").fill_(1 << 62)  # the block the copy had, if any
                side.synchronize()
                assert np.array_equal(got.cpu().numpy(), want), (label, frames, "side stream")
                assert bool((reuse == (1 << 62)).all())
                torch.cuda.current_stream().wait_stream(side)
            assert int(table3[:, 2].min()) == CANARIES["int64"] == int(table3[:, 2].max())
    finally:
        plan.close()


# ---- plan runs on views of exactly the plan's extent ------------------------------------------------------------------------------

def ragged(c, first):
    """five streams of different lengths out of the corpus, `first` the stream the first comes from -> list of int16 [n_i, ch]"""
    lengths = [c["n"], 7, c["spb"] + 3, 1, 2 * c["spb"]]
    return [c["pcm"][first + i][:v].copy() for i, v in enumerate(lengths)]


def ragged_table(engine, c, pcms, pcm_span):
    """offsets out of order with gaps; data_size is the image's own size; pcm_span(i): the elements stream i takes in the input"""
    d = np.zeros(len(pcms), dtype=STREAM_DESC_DTYPE)
    pos_p, pos_d = 1, 3
    for i in (3, 0, 4, 1, 2):
        d["pcm_offset"][i], d["data_offset"][i] = pos_p, pos_d
        d["num_samples"][i] = len(pcms[i])
        d["data_size"][i] = engine.encoded_size(c["param"], len(pcms[i]))
        pos_p += pcm_span(i) + 1 + i % 3
        pos_d += int(d["data_size"][i]) + 5 + i
    return d


def outside_images(torch, data, d, label):
    keep = torch.ones(data.numel(), dtype=torch.bool, device=data.device)
    for o, s in zip(d["data_offset"], d["data_size"]):
        keep[int(o):int(o) + int(s)] = False
    assert bool((data[keep] == CANARIES["uint8"]).all()), (label, "a byte between the images was written")


def carried_oracle(c, runs):
    """runs: lists of pcms, encoded one after the other on the same encoders -> per run the images"""
    lanes = [ob.fresh_lanes(c["ch"]) for _ in runs[0]]
    return [[ob.encode(p, c["bits"], MBS, 48000, False, 0, lanes=lanes[i], reset_idx=False) for i, p in enumerate(pcms)] for pcms in runs]


def exact_view(torch, extent, dtype, lead):
    """a view of exactly `extent` canaries with canaries in front of and behind it"""
    return embedded(torch, canary_buffer(torch, extent, dtype, "cuda"), lead, 0)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_interleaved_plan_runs_on_exact_extent_views(engine, case):
    """EncodePlan.run twice over carried state, then DecodePlan.run of the second run's images: pcm, data, state and the decoded
    pcm are views of exactly run_extent elements, canaries on both sides and in the gaps between the streams"""
    import torch
    c = corpus(*case)
    ch = c["ch"]
    runs = [ragged(c, 0), ragged(c, STREAMS)]
    want = carried_oracle(c, runs)
    d = ragged_table(engine, c, runs[0], lambda i: len(runs[0][i]) * ch)
    e_pcm, e_data = run_extent("interleaved", d, ch), run_extent("images", d)
    sbuf, state = embedded(torch, torch.zeros((STREAMS * ch, 10), dtype=torch.int32, device="cuda"), 7, 0)
    plan = engine.encode_plan(c["param"], d)
    try:
        for k, pcms in enumerate(runs):
            pbuf, pcm = exact_view(torch, e_pcm, torch.int16, 1)
            for i, p in enumerate(pcms):
                o = int(d["pcm_offset"][i])
                pcm[o:o + p.size] = torch.from_numpy(p.reshape(-1)).cuda()
            before = pbuf.clone()
            dbuf, data = exact_view(torch, e_data, torch.uint8, 3)
            assert pcm.numel() == e_pcm and data.numel() == e_data and pcm.data_ptr() % 4 == 2
            plan.run(pcm, data, state)
            torch.cuda.synchronize()
            host = data.cpu().numpy()
            for i, w in enumerate(want[k]):
                o = int(d["data_offset"][i])
                assert bytes(host[o:o + len(w)]) == w and len(w) == int(d["data_size"][i]), ("run", k, "stream", i)
            outside_images(torch, data, d, ("run", k))
            untouched(torch, dbuf, data, "data")
            untouched(torch, sbuf, state, "state")
            assert torch.equal(pbuf, before), "the input changed"
    finally:
        plan.close()
    dec = engine.decode_plan(parse_header(want[1][0][:31]), d, True)
    try:
        obuf, out = exact_view(torch, e_pcm, torch.int16, 1)
        dec.run(data, out)
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        written = np.zeros(e_pcm, dtype=bool)
        for i, w in enumerate(want[1]):
            o, size = int(d["pcm_offset"][i]), len(runs[1][i]) * ch
            assert np.array_equal(host[o:o + size].reshape(-1, ch), ob.decode(w)[0]), ("decode", i)
            written[o:o + size] = True
        assert (host[~written] == CANARIES["int16"]).all(), "a sample between the streams was written"
        untouched(torch, obuf, out, "pcm")
    finally:
        dec.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_uniform_encode_and_reconstruct_on_contiguous_views_at_an_offset(engine, case):
    """encode_uniform and reconstruct_uniform need contiguous PCM; a contiguous view on an odd 2-byte alignment, and a state table
    inside canaries, are as good as tensors of their own"""
    import torch
    c = corpus(*case)
    ch = c["ch"]
    pbuf, pcm = embedded(torch, torch.from_numpy(c["pcm"][:STREAMS].copy()).cuda(), 1, 0)
    sbuf, state = embedded(torch, torch.zeros((STREAMS * ch, 10), dtype=torch.int32, device="cuda"), 7, 0)
    assert pcm.is_contiguous() and state.is_contiguous() and pcm.data_ptr() % 4 == 2
    before = pbuf.clone()
    img, size = engine.encode_uniform(pcm, c["param"], state=state)
    host = img.cpu().numpy()
    assert size == c["size"] and all(bytes(host[s, :size]) == c["images"][s] for s in range(STREAMS))
    rec, stats = engine.reconstruct_uniform(pcm, c["param"])
    assert np.array_equal(rec.cpu().numpy(), np.stack(c["decoded"][:STREAMS]))
    lines = [ob.stats_line(tuple(float(v) for v in row)) for row in stats.cpu().numpy()]  # the contract of these doubles: `aad -c`'s line
    assert lines == [ob.stats_line(ob.error_stats(c["pcm"][s], c["decoded"][s])) for s in range(STREAMS)]
    untouched(torch, sbuf, state, "state")
    assert torch.equal(pbuf, before), "the input changed"


def planar_flat(torch, c, pcms, d, cs, dtype, e_x):
    """the plan's input: every stream's channel rows at pcm_offset + c * cs of an exact-extent view"""
    xbuf, x = exact_view(torch, e_x, dtype, 1)
    for i, p in enumerate(pcms):
        for k in range(c["ch"]):
            o = int(d["pcm_offset"][i]) + k * cs
            row = torch.from_numpy(np.ascontiguousarray(p[:, k])).cuda()
            x[o:o + len(p)] = row if dtype == torch.int16 else row.to(torch.float32) / 32768.0
    return xbuf, x


def error_stats(pcms, decoded, ch):
    out = np.zeros((len(pcms), ch, 4), dtype=np.int64)
    for i, (p, q) in enumerate(zip(pcms, decoded)):
        e = np.abs(p.astype(np.int64) - q.astype(np.int64))
        out[i, :, 0], out[i, :, 1], out[i, :, 2], out[i, :, 3] = (e * e).sum(0), e.sum(0), e.max(0), len(p)
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_planar_plan_runs_on_exact_extent_views(engine, case):
    """PlanarEncodePlan.run, and PlanarReconstructPlan.run twice over carried state with out and stats: every argument a view of
    exactly the plan's extent; the output's stream stride is no multiple of its channel stride"""
    import torch
    c = corpus(*case)
    ch, param = c["ch"], c["param"]
    runs = [ragged(c, 0), ragged(c, STREAMS)]
    want = carried_oracle(c, runs)
    longest = max(len(p) for p in runs[0])
    cs = longest + 3
    d = ragged_table(engine, c, runs[0], lambda i: (ch - 1) * cs + len(runs[0][i]))
    e_x, e_data = run_extent("planar", d, ch, channel_stride=cs), run_extent("images", d)
    in_dtype = torch.float32 if c["bits"] == 2 else torch.int16
    # planar encode: fresh encoders
    plan = engine.planar_encode_plan(param, d, cs, in_dtype)
    try:
        xbuf, x = planar_flat(torch, c, runs[0], d, cs, in_dtype, e_x)
        dbuf, data = exact_view(torch, e_data, torch.uint8, 3)
        plan.run(x, data)
        torch.cuda.synchronize()
        host = data.cpu().numpy()
        for i, w in enumerate(want[0]):
            o = int(d["data_offset"][i])
            assert bytes(host[o:o + len(w)]) == w, ("planar encode", i)
        outside_images(torch, data, d, "planar encode")
        untouched(torch, dbuf, data, "data")
    finally:
        plan.close()
    # planar reconstruct: rows, statistics and carried state
    ocs, oss = longest + 2, ch * (longest + 2) + 5
    e_out = run_extent("planar_out", d, ch, channel_stride=ocs, stream_stride=oss)
    sbuf, state = embedded(torch, torch.zeros((STREAMS * ch, 10), dtype=torch.int32, device="cuda"), 7, 0)
    plan = engine.planar_reconstruct_plan(param, d, cs, in_dtype, torch.float32, oss, ocs)
    try:
        for k, pcms in enumerate(runs):
            xbuf, x = planar_flat(torch, c, pcms, d, cs, in_dtype, e_x)
            dbuf, data = exact_view(torch, e_data, torch.uint8, 3)
            obuf, out = exact_view(torch, e_out, torch.float32, 1)
            tbuf, stats = embedded(torch, canary_buffer(torch, STREAMS * ch * 4, torch.int64, "cuda").view(STREAMS, ch, 4), 3, 0)
            assert stats.is_contiguous() and out.numel() == e_out
            plan.run(x, data, out, state, stats=stats)
            torch.cuda.synchronize()
            host, rows = data.cpu().numpy(), out.cpu().numpy()
            decoded = [ob.decode(w)[0] for w in want[k]]
            written = np.zeros(e_out, dtype=bool)
            for i, w in enumerate(want[k]):
                o = int(d["data_offset"][i])
                assert bytes(host[o:o + len(w)]) == w, ("reconstruct run", k, "image", i)
                for ci in range(ch):
                    o = i * oss + ci * ocs
                    expect = decoded[i][:, ci].astype(np.float32) / np.float32(32768.0)
                    assert np.array_equal(rows[o:o + len(expect)].view(np.uint32), expect.view(np.uint32)), ("run", k, "row", i, ci)
                    written[o:o + len(expect)] = True
            assert (rows.view(np.uint32)[~written] == CANARIES["float32"]).all(), "an element outside the rows was written"
            assert np.array_equal(stats.cpu().numpy(), error_stats(pcms, decoded, ch)), ("run", k, "stats")
            outside_images(torch, data, d, ("reconstruct run", k))
            for name, b, v in (("data", dbuf, data), ("out", obuf, out), ("stats", tbuf, stats), ("state", sbuf, state)):
                untouched(torch, b, v, name)
    finally:
        plan.close()


# ---- planar and window-reconstruct inputs as views --------------------------------------------------------------------------------

def planar_views(torch, c):
    """(label, buffer, view [5, C, n]) of the planar int16 batch: at a storage offset with a padded pitch; with a stream stride that is
    no multiple of the channel stride; with overlapping streams (the expected values are whatever the view shows)"""
    ch, n = c["ch"], c["n"]
    x = torch.from_numpy(np.ascontiguousarray(c["pcm"][:STREAMS].transpose(0, 2, 1))).cuda()
    out = [("offset and pitch",) + embedded(torch, x, 3, 7)]
    out.append(("stream stride not a multiple of the channel stride",) + laid(torch, x, (ch * (n + 7) + 5, n + 7, 1), 1))
    flat = torch.from_numpy(synth_pcm(1, (STREAMS + ch + 2) * (n + 9), 1, seed=77)[0].reshape(-1)).cuda()
    over = torch.as_strided(flat, (STREAMS, ch, n), (n // 3 + 1, n + 5, 1), 5)
    assert over.stride(0) < ch * n
    out.append(("overlapping streams", None, over))
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_planar_entry_points_read_views_in_place(engine, case):
    import torch
    c = corpus(*case)
    ch, n, spb, bits, param = c["ch"], c["n"], c["spb"], c["bits"], c["param"]
    mixed_bits = [4, 2, 3, 2, 4]
    make_param = lambda b: make_parameter(ch, b, MBS, 48000, False, 0)
    frames = spb + 3
    win = np.array([(0, 0), (4, spb - 1), (2, n - 17), (1, n), (STREAMS, 0), (3, 5)], dtype=np.int64)
    d_win = torch.from_numpy(win).cuda()
    for label, buffer, x in planar_views(torch, c):
        assert x.stride(-1) == 1 and not x.is_contiguous()
        shown = x.cpu().numpy()  # [5, C, n]: what the view shows is what must be encoded
        plain = x.contiguous()
        images = [ob.encode(shown[i].T, bits, MBS) for i in range(STREAMS)]
        decoded = [ob.decode(w)[0] for w in images]
        want_stats = error_stats([shown[i].T for i in range(STREAMS)], decoded, ch)
        out, sizes = engine.encode_planar(x, param)
        host = out.cpu().numpy()
        assert all(bytes(host[i, :sizes[i]]) == images[i] for i in range(STREAMS)), (label, "encode_planar")
        assert torch.equal(out, engine.encode_planar(plain, param)[0]), (label, "encode_planar against the contiguous call")
        y, img2, sizes2, stats = engine.reconstruct_planar(x, param, return_images=True, return_stats=True)
        assert np.array_equal(y.cpu().numpy(), np.stack([q.T for q in decoded])), (label, "reconstruct_planar rows")
        assert torch.equal(img2, out) and sizes2 == sizes and np.array_equal(stats.cpu().numpy(), want_stats), (label, "reconstruct_planar")
        assert torch.equal(y, engine.reconstruct_planar(plain, param)), (label, "reconstruct_planar against the contiguous call")
        assert np.array_equal(engine.codec_error(x, param).cpu().numpy(), want_stats), (label, "codec_error")
        mout, msizes = engine.encode_planar_mixed(x, make_param, mixed_bits)
        mhost = mout.cpu().numpy()
        assert all(bytes(mhost[i, :msizes[i]]) == ob.encode(shown[i].T, mixed_bits[i], MBS) for i in range(STREAMS)), (label, "encode_planar_mixed")
        rows = engine.reconstruct_windows(x, d_win, frames, param).cpu().numpy()
        for w, (s, f) in enumerate(win.tolist()):
            expect = np.zeros((ch, frames), dtype=np.int16)
            if s < STREAMS and f < n:
                crop = shown[s][:, f:f + frames]
                expect[:, :crop.shape[1]] = ob.decode(ob.encode(crop.T, bits, MBS))[0].T
            assert np.array_equal(rows[w], expect), (label, "reconstruct_windows", w)
        assert np.array_equal(rows, engine.reconstruct_windows(plain, d_win, frames, param).cpu().numpy()), (label, "windows against the contiguous call")
        wbuf, wview = embedded(torch, d_win, 1, 1)  # the window table as a view while the corpus stays plain
        assert np.array_equal(rows, engine.reconstruct_windows(plain, wview, frames, param).cpu().numpy()), (label, "windows as a view")
        untouched(torch, wbuf, wview, "windows")
        if buffer is not None:
            untouched(torch, buffer, x, label)


def test_expanded_mono_rows_are_refused_without_a_run(refusing):
    import torch
    c = corpus(2, 4)
    mono = torch.zeros((STREAMS, 1, c["n"]), dtype=torch.int16, device="cuda")
    x = mono.expand(STREAMS, 2, c["n"])
    win = torch.zeros((3, 2), dtype=torch.int64, device="cuda")
    for call in (lambda: refusing.encode_planar(x, c["param"]), lambda: refusing.reconstruct_planar(x, c["param"]),
                 lambda: refusing.codec_error(x, c["param"]), lambda: refusing.reconstruct_windows(x, win, 17, c["param"]),
                 lambda: refusing.encode_planar_mixed(x, lambda b: make_parameter(2, b, MBS), [4] * STREAMS)):
        with pytest.raises(ValueError, match=r"channel stride 0 \(stride\(1\)\)"):
            call()


# ---- the step pipeline at small rings ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ring", [2, 4])
def test_pipeline_at_small_rings(ring):
    """12 steps with a different batch each: every step's decoded PCM and the ring's last images are the oracle's for that step's
    batch - the half-ring wait index is the part that changes with `ring`"""
    import torch
    from aad_amd.engine import Engine, EncodeDecodePipeline
    c = corpus(2, 4)
    steps = 12
    e1, e2 = Engine(0, stream=torch.cuda.Stream()), Engine(0, stream=torch.cuda.Stream())
    try:
        batches = [synth_pcm(STREAMS, c["n"], 2, seed=9100 + k) for k in range(steps)]
        d_in = [torch.from_numpy(b).cuda() for b in batches]
        d_out = [torch.zeros_like(t) for t in d_in]
        pipe = EncodeDecodePipeline(e1, e2, c["param"], STREAMS, c["n"], ring=ring)
        try:
            for k in range(steps):
                pipe.step(d_in[k], d_out[k])
            torch.cuda.synchronize()
            for k in range(steps):
                want = [ob.encode(batches[k][s], 4, MBS) for s in range(STREAMS)]
                got = d_out[k].cpu().numpy()
                for s in range(STREAMS):
                    assert np.array_equal(got[s], ob.decode(want[s])[0]), (ring, "step", k, "stream", s)
                if k >= steps - ring:
                    img = pipe.images[k % ring].cpu().numpy()
                    assert all(bytes(img[s, :pipe.enc.image_size]) == want[s] for s in range(STREAMS)), (ring, "step", k, "images")
        finally:
            pipe.close()
    finally:
        e1.close()
        e2.close()


# ---- refusals: none of them may reach a run ---------------------------------------------------------------------------------------

def refuse(call, good, rules, label):
    from test_engine_tensor_contract import spoil
    for arg, names in rules.items():
        for rule in names:
            bad = dict(good)
            bad[arg] = spoil(good[arg], rule)
            with pytest.raises(ValueError, match=r"\b%s\b" % arg):
                call(**bad)
                raise AssertionError((label, arg, rule, "was accepted"))


ROWS = ("dtype", "device", "stride", "short")
STATE = ("dtype", "device", "rank", "stride", "short")
TABLE = ("dtype", "device", "rank", "stride", "noncontiguous", "short")
VIEW = ("dtype", "device", "rank", "stride")
WINDOWS = ("dtype", "device", "rank", "short")


def test_plan_runs_refuse_bad_tensors_before_the_library(refusing):
    import torch
    e, c = refusing, corpus(2, 4)
    ch, param = c["ch"], c["param"]
    pcms = ragged(c, 0)
    zeros = lambda count, dtype: torch.zeros(count, dtype=dtype, device="cuda")
    state = torch.zeros((STREAMS * ch, 10), dtype=torch.int32, device="cuda")
    d = ragged_table(e, c, pcms, lambda i: len(pcms[i]) * ch)
    good = dict(pcm=zeros(run_extent("interleaved", d, ch), torch.int16), data=zeros(run_extent("images", d), torch.uint8), state=state)
    plan = e.encode_plan(param, d)
    refuse(lambda pcm, data, state: plan.run(pcm, data, state), good, dict(pcm=ROWS, data=ROWS, state=STATE), "EncodePlan.run")
    plan.close()
    plan = e.decode_plan(parse_header(c["images"][0][:31]), d, True)
    refuse(lambda pcm, data, state: plan.run(data, pcm), good, dict(pcm=ROWS, data=ROWS), "DecodePlan.run")
    plan.close()
    longest = max(len(p) for p in pcms)
    cs, ocs, oss = longest + 3, longest + 2, ch * (longest + 2) + 5
    d = ragged_table(e, c, pcms, lambda i: (ch - 1) * cs + len(pcms[i]))
    good = dict(x=zeros(run_extent("planar", d, ch, channel_stride=cs), torch.int16), data=zeros(run_extent("images", d), torch.uint8), state=state,
                out=zeros(run_extent("planar_out", d, ch, channel_stride=ocs, stream_stride=oss), torch.float32),
                stats=torch.zeros((STREAMS, ch, 4), dtype=torch.int64, device="cuda"))
    plan = e.planar_encode_plan(param, d, cs, torch.int16)
    refuse(lambda x, data, state, out, stats: plan.run(x, data, state), good, dict(x=ROWS, data=ROWS, state=STATE), "PlanarEncodePlan.run")
    plan.close()
    plan = e.planar_reconstruct_plan(param, d, cs, torch.int16, torch.float32, oss, ocs)
    refuse(lambda x, data, state, out, stats: plan.run(x, data, out, state, stats=stats), good,
           dict(x=ROWS, data=ROWS, out=ROWS, state=STATE, stats=TABLE), "PlanarReconstructPlan.run")
    plan.close()
    frames, n_win = 17, 4
    win = torch.zeros((n_win, 2), dtype=torch.int64, device="cuda")
    views = [torch.zeros((n_win, 3), dtype=torch.int64, device="cuda")[:, :2], torch.zeros((2, n_win), dtype=torch.int64, device="cuda").t()]
    wgood = dict(x=good["x"], windows=win, out=torch.zeros((n_win, ch, frames), device="cuda"), stats=torch.zeros((n_win, ch, 4), dtype=torch.int64, device="cuda"),
                 data=torch.zeros((n_win, round64(e.encoded_size(param, frames))), dtype=torch.uint8, device="cuda"))
    plan = e.window_reconstruct_plan(param, d, cs, torch.int16)
    refuse(lambda x, windows, out, stats, data: plan.run(x, windows, frames, out=out, data=data, stats=stats), wgood,
           dict(x=ROWS, windows=WINDOWS, out=VIEW + ("short",), data=VIEW + ("short",), stats=TABLE), "WindowReconstructPlan.run")
    for v in views:
        with pytest.raises(ValueError, match="ordered=False"):
            plan.run(wgood["x"], v, frames, ordered=False)
    plan.close()
    img = image_rows(torch, c)
    dgood = dict(data=img, windows=win, out=wgood["out"], stats=wgood["stats"])
    plan = e.uniform_window_decode_plan(parse_header(c["images"][0][:31]), 2 * STREAMS, img.stride(0), c["size"])
    refuse(lambda data, windows, out, stats: plan.run(data, windows, frames, out=out, stats=stats), dgood,
           dict(data=("dtype", "device", "stride"), windows=WINDOWS, out=TABLE, stats=TABLE), "WindowDecodePlan.run")
    with pytest.raises(ValueError, match="data: the run touches"):
        plan.run(img.reshape(-1)[:-(img.shape[1] - c["size"]) - 1], win, frames)  # one byte short of the last image
    for v in views:
        with pytest.raises(ValueError, match="ordered=False"):
            plan.run(img, v, frames, ordered=False)
    plan.close()


def test_entry_points_refuse_bad_tensors_before_the_library(refusing):
    import torch
    e, c = refusing, corpus(2, 4)
    ch, n, param, size = c["ch"], c["n"], c["param"], c["size"]
    state = torch.zeros((STREAMS * ch, 10), dtype=torch.int32, device="cuda")
    pcm = torch.from_numpy(c["pcm"][:STREAMS].copy()).cuda()
    contiguous = ("dtype", "device", "rank", "stride", "noncontiguous")
    refuse(lambda pcm, state: e.encode_uniform(pcm, param, state), dict(pcm=pcm, state=state), dict(pcm=contiguous, state=STATE), "encode_uniform")
    refuse(lambda pcm, state: e.reconstruct_uniform(pcm, param), dict(pcm=pcm, state=state), dict(pcm=contiguous), "reconstruct_uniform")
    x = pcm.transpose(1, 2).contiguous()
    win = torch.zeros((4, 2), dtype=torch.int64, device="cuda")
    for fn in ("encode_planar", "reconstruct_planar", "codec_error"):
        refuse(lambda x, state: getattr(e, fn)(x, param, state=state), dict(x=x, state=state), dict(x=VIEW, state=STATE), fn)
    refuse(lambda x, state: e.encode_planar_mixed(x, lambda b: make_parameter(ch, b, MBS), [4] * STREAMS), dict(x=x, state=state), dict(x=VIEW), "encode_planar_mixed")
    for fn in ("reconstruct_windows", "codec_error_windows"):
        refuse(lambda corpus, windows: getattr(e, fn)(corpus, windows, 17, param), dict(corpus=x, windows=win), dict(corpus=VIEW, windows=WINDOWS), fn)
    img = image_rows(torch, c)
    refuse(lambda data, windows: e.decode_uniform(data, size), dict(data=img, windows=win), dict(data=VIEW), "decode_uniform")
    for fn in ("decode_windows", "decode_windows_mixed"):
        refuse(lambda data, windows: getattr(e, fn)(data, size, windows, 17), dict(data=img, windows=win), dict(data=VIEW, windows=WINDOWS), fn)
    refuse(lambda data, windows: e.window_levels(data, size, windows, 17), dict(data=img, windows=win), dict(data=VIEW, windows=WINDOWS), "window_levels")
    for data in (img, img[:, :size], img[::2]):
        width = data.shape[1]
        for call in (lambda: e.decode_uniform(data, width + 1), lambda: e.decode_windows(data, width + 1, win, 17),
                     lambda: e.decode_windows_mixed(data, width + 1, win, 17), lambda: e.window_levels(data, width + 1, win, 17)):
            with pytest.raises(ValueError, match="data: an image of %d bytes" % (width + 1)):
                call()
    with pytest.raises(ValueError, match=r"pcm_list\[0\]"):
        e.encode_host([np.zeros((50, 1), dtype=np.int16)], param)
    with pytest.raises(ValueError, match=r"pcm_list\[1\]"):
        e.reconstruct_host([np.zeros((50, 2), dtype=np.int16), np.zeros(50, dtype=np.int16)], param)
    with pytest.raises(ValueError, match="state"):
        e.encode_host([np.zeros((50, 2), dtype=np.int16)], param, state=np.zeros((2, 10), dtype=np.int32))
