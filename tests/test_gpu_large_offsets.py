"""Device paths with streams and waves past 4 GiB: every offset the kernels and the host staging take is 64-bit, and these tests put
real data on both sides of the places where a 32-bit intermediate would wrap.  A narrowed offset keeps every address inside the
same allocation, so it cannot fault: it reads or writes the wrong stream's bytes, and only a bit-exact comparison sees it.  Every
result is compared with the oracle (tests/oracle_binding.py) or the segmented definition (tests/segment_oracle.py), and every
stream's inputs differ (seed and length), so a stream that picks up a neighbour's data, or data 2^32 elements away, fails.

  test                                   device paths                                            placements asserted
  -------------------------------------  ------------------------------------------------------  ------------------------------------------
  test_encode_plans                      encode_streams_kernel: quad, quad dual / single trial   PCM: streams across elements 2^31 and 2^32
                                         lanes, dense (per-lane stores; the byte ring under      (bytes 2^32 and 2^33), one wholly above
                                         AAD_HIP_ENCODE_RING=2), uniform and table layouts       2^32; images across bytes 2^31 and 2^32,
  test_decode_plans                      split (LDS residuals), quad-fused, dense per-lane,      one wholly above 2^32 - uniform layout
                                         sector-tiled decoders; uniform and table branches       (stride 2^29) and a shuffled table with
  test_reconstruct_plans                 encode + decode + compare kernels, decoded and          neighbours a few units apart at every
                                         residual output, sequential statistics                  boundary
  test_segmented_plans                   segmented encoder (chain table), segmented
                                         reconstruction; (L, W) = (1, 0), (4, 2), (16, 3)
  test_reconstruct_batch                 AADHip_ReconstructBatch at the default wave budget      one wave of > 2^32 PCM elements (~8.8 GiB):
  test_segmented_reconstruct_batch       AADHip_SegmentedReconstructBatch, same                  rows across elements 2^31 and 2^32
  test_segmented_encode_batch            AADHip_SegmentedEncodeBatch (staging rows / spots)
  test_one_stream_past_4gib              segmented encoder L = 1, W = 0 on one stream of          in-stream offsets first * ch past 2^31 and
                                         2^32 - 1 stereo frames; every decode mapping, uniform    2^32 elements (PCM 16 GiB), block offsets
                                         and table branch                                        past 2^31 and 2^32 bytes (image 4.1 GiB)

Device memory: read before each test; a test skips only when the free memory is below its need plus 8 GiB (an MI355X has far more).
Each test frees its buffers, empties torch's cache and closes its Engine (the context's grow-only blocks go with it)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import oracle_binding as ob
import segment_oracle as so
from aad_amd.capi import (AADHipSegmentation, RECONSTRUCT_DECODED, RECONSTRUCT_RESIDUAL, STREAM_DESC_DTYPE, make_parameter)

pytestmark = pytest.mark.gpu

B29, B31, B32, B33 = 1 << 29, 1 << 31, 1 << 32, 1 << 33
GIB = 1 << 30
MARGIN = 320                 # canary units (int16 elements / bytes) on either side of every stream
PCM_CANARY, OUT_CANARY, IMG_CANARY = 0x1D2B, 0x5A5A, 0xA5
PLAN_UNITS = B32 + B29 + (1 << 20)  # PCM elements (~9 GiB) and image bytes (~4.5 GiB) of the plan tests
MAPPINGS = ["auto", "dense", "dense-tiled", "quad", "quad-fused"]
CONFIGS = {"mono": (1, False), "stereo": (2, False), "ms": (2, True), "ch8": (8, False)}


def _round_up(v, a):
    return (v + a - 1) // a * a


def _need(gib):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < (gib + 8) * GIB:
        pytest.skip("needs %d GiB of free device memory plus 8 GiB headroom, %.1f GiB free" % (gib, free / GIB))


@pytest.fixture
def engine():
    import torch
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ---- windows: a stream's units and a canary margin on either side ---------------------------------------------------------------

class Windows:
    """The union of [start - MARGIN, start + length + MARGIN) over a batch's spans (start, length) of one buffer, as disjoint
    intervals: filled with a canary, the streams written on top, read back in one piece and compared with what it must hold."""

    def __init__(self, spans):
        ivs = sorted((max(0, s - MARGIN), s + n + MARGIN) for s, n in spans)
        merged = []
        for a, b in ivs:
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        self.intervals = [(a, b) for a, b in merged]
        self.base = np.cumsum([0] + [b - a for a, b in self.intervals])

    def where(self, start):
        """position of buffer unit `start` in the gathered array"""
        k = max(i for i, (a, _) in enumerate(self.intervals) if a <= start)
        return int(self.base[k] + start - self.intervals[k][0])

    def expect(self, canary, dtype, streams):
        """the gathered array as it must be: the canary, with every (start, values) of `streams` on top"""
        out = np.full(int(self.base[-1]), canary, dtype=dtype)
        for start, values in streams:
            p = self.where(start)
            out[p:p + len(values)] = values
        return out

    def fill(self, buf, canary, streams=()):
        import torch
        for a, b in self.intervals:
            buf[a:b].fill_(canary)
        for start, values in streams:
            buf[start:start + len(values)].copy_(torch.from_numpy(np.require(values, requirements=["C", "W"])))

    def read(self, buf):
        import torch
        return torch.cat([buf[a:b] for a, b in self.intervals]).cpu().numpy()


def _first_bad(got, want, w, what):
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    p = int(bad[0])
    k = max(i for i in range(len(w.intervals)) if w.base[i] <= p)
    return "%s: %d units differ, first at buffer unit %d" % (what, bad.size, w.intervals[k][0] + p - int(w.base[k]))


# ---- layouts --------------------------------------------------------------------------------------------------------------------

def _uniform_offsets(count, size, align):
    """arithmetic progression of stride 2^29 units: stream 3 lies across 2^31, stream 7 across 2^32, stream 8 wholly above 2^32
    (and 2^32 units after stream 0: a 32-bit wrap of its offset lands on stream 0's)"""
    assert count == 9
    base = B29 - _round_up(size // 2, align)
    return [base + i * B29 for i in range(count)]


def _table_offsets(sizes, align, rng):
    """Offsets of spans `sizes` (units) in a shuffled order: around each of 2^31 and 2^32 three neighbours a few units apart - one
    ending just below, one across, one starting just above -, one near 0, one near 2^30 and one well above 2^32."""
    assert len(sizes) == 9
    order = [int(i) for i in rng.permutation(9)]
    off = [0] * 9
    gap = lambda: align * int(rng.integers(1, 6))
    for k, x in enumerate((B31, B32)):
        lo, mid, hi = order[3 * k:3 * k + 3]
        off[mid] = (x - sizes[mid] // 2) // align * align
        off[lo] = (off[mid] - gap() - sizes[lo]) // align * align
        off[hi] = _round_up(off[mid] + sizes[mid] + gap(), align)
    off[order[6]] = _round_up(MARGIN + int(rng.integers(0, 4096)), align)
    off[order[7]] = _round_up((1 << 30) + int(rng.integers(0, 1 << 20)), align)
    off[order[8]] = _round_up(B32 + (1 << 28) + int(rng.integers(0, 1 << 20)), align)
    return off


def _assert_placement(offsets, sizes, limit):
    """the boundaries each layout exists for: real data on both sides of 2^31 and 2^32 units, a stream wholly above 2^32, and
    every span (with its canary margin) inside the buffer"""
    spans = list(zip(offsets, sizes))
    for x in (B31, B32):
        assert any(o < x < o + n for o, n in spans), ("no stream across", x)
    assert any(o > B32 for o, _ in spans), "no stream wholly above 2^32"
    assert all(o >= MARGIN and o + n + MARGIN <= limit for o, n in spans)
    s = sorted(spans)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(s, s[1:])), "streams overlap"


class Batch:
    """Nine streams of one parameter set placed in the plan buffers: PCM (int16 elements, 16-byte aligned for the sector-tiled
    decoder) and images (bytes; uniform layout: 128-byte aligned - the ring's 64-byte sectors and the 3-bit tiled rows' code
    phase -, table layout: any byte phase)."""

    def __init__(self, layout, bits, cfg, frames, seed, image_size):
        ch, ms = CONFIGS[cfg]
        self.layout, self.bits, self.ch, self.ms = layout, bits, ch, ms
        rng = np.random.default_rng(seed)
        self.frames = list(frames)
        self.pcm = [np.ascontiguousarray(_synth(int(rng.integers(0, 1 << 30)), n, ch, i)) for i, n in enumerate(self.frames)]
        self.sizes = [image_size(n) for n in self.frames]
        elems = [n * ch for n in self.frames]
        if layout == "uniform":
            assert len(set(self.frames)) == 1
            self.pcm_off = _uniform_offsets(9, elems[0], 8)
            self.img_off = _uniform_offsets(9, self.sizes[0], 128)
        else:
            assert len(set(self.frames)) == 9
            self.pcm_off = _table_offsets(elems, 8, rng)
            self.img_off = _table_offsets(self.sizes, 1, rng)
        _assert_placement(self.pcm_off, elems, PLAN_UNITS)
        _assert_placement(self.img_off, self.sizes, PLAN_UNITS)
        assert all(o % 8 == 0 for o in self.pcm_off)
        self.descs = np.zeros(9, dtype=STREAM_DESC_DTYPE)
        self.descs["pcm_offset"], self.descs["data_offset"] = self.pcm_off, self.img_off
        self.descs["data_size"], self.descs["num_samples"] = self.sizes, self.frames
        self.pcm_win = Windows(zip(self.pcm_off, elems))
        self.img_win = Windows(zip(self.img_off, self.sizes))

    def param(self, trials=0):
        return make_parameter(self.ch, self.bits, 1024, 48000, self.ms, trials)

    def pcm_streams(self):
        return [(o, p.reshape(-1)) for o, p in zip(self.pcm_off, self.pcm)]

    def put_pcm(self, buf):
        self.pcm_win.fill(buf, PCM_CANARY, self.pcm_streams())

    def check_pcm_untouched(self, buf, what):
        bad = _first_bad(self.pcm_win.read(buf), self.pcm_win.expect(PCM_CANARY, np.int16, self.pcm_streams()), self.pcm_win, what)
        assert bad is None, bad

    def check_images(self, buf, images, what):
        want = self.img_win.expect(IMG_CANARY, np.uint8, [(o, np.frombuffer(b, dtype=np.uint8)) for o, b in zip(self.img_off, images)])
        bad = _first_bad(self.img_win.read(buf), want, self.img_win, what)
        assert bad is None, bad

    def check_out(self, buf, outs, what):
        want = self.pcm_win.expect(OUT_CANARY, np.int16, [(o, y.reshape(-1)) for o, y in zip(self.pcm_off, outs)])
        bad = _first_bad(self.pcm_win.read(buf), want, self.pcm_win, what)
        assert bad is None, bad


def _synth(seed, frames, ch, i):
    from aad_amd.synth import synth_pcm
    return synth_pcm(1, frames, ch, seed=seed, kind="noise" if i % 3 == 1 else "music")[0]


def _plan_frames(layout, spb, blocks):
    """distinct ragged lengths (table) or one ragged length (uniform) of about `blocks` blocks"""
    if layout == "uniform":
        return [blocks * spb + 123] * 9
    return [spb * (blocks - 1 + i % 3) + 37 * i + 5 for i in range(9)]


def _plan_buffers(need_pcm=True, need_out=True):
    import torch
    pcm = torch.empty(PLAN_UNITS, dtype=torch.int16, device="cuda") if need_pcm else None
    img = torch.empty(PLAN_UNITS, dtype=torch.uint8, device="cuda")
    out = torch.empty(PLAN_UNITS, dtype=torch.int16, device="cuda") if need_out else None
    return pcm, img, out


def _encoded_size(engine, bits, cfg):
    ch, ms = CONFIGS[cfg]
    param = make_parameter(ch, bits, 1024, 48000, ms, 0)
    return lambda n: engine.encoded_size(param, n)


# ---- 1. device-resident plans with hand-made tables -------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("bits", [4, 3, 2])
def test_encode_plans(engine, monkeypatch, bits, cfg):
    """AADHip_EncodePlanRun with every mapping (quad, quad-fused, dense, dense-tiled, auto), trials 0 and 2 under the dual and the
    single trial lanes, on a uniform layout (the table-free kernel path) and a shuffled table whose PCM crosses elements 2^31 and
    2^32 and whose images cross bytes 2^31 and 2^32; mono / stereo also through the dense encoders' byte ring
    (AAD_HIP_ENCODE_RING=2) on the uniform layout, whose images sit on 64-byte boundaries.  The image buffer's canary around
    every image and the PCM buffer's around every stream must survive."""
    import torch
    from aad_amd.engine import Engine
    _need(14)
    ch, ms = CONFIGS[cfg]
    rc, block_size, spb = ob.geometry(1024, ch, bits)
    assert rc == 0
    pcm, img, _ = _plan_buffers(need_out=False)
    for layout in ("uniform", "table"):
        b = Batch(layout, bits, cfg, _plan_frames(layout, spb, 3), 4100 + 10 * bits + ch + ms, _encoded_size(engine, bits, cfg))
        b.put_pcm(pcm)
        for trials in (0, 2):
            want = [ob.encode(p, bits, 1024, 48000, ms, trials) for p in b.pcm]
            assert [len(w) for w in want] == b.sizes
            for mapping in MAPPINGS:
                for lanes in (("dual", "single") if trials else ("dual",)):
                    b.img_win.fill(img, IMG_CANARY)
                    engine.set_mapping(mapping, lanes)
                    plan = engine.encode_plan(b.param(trials), b.descs)
                    plan.run(pcm, img)
                    torch.cuda.synchronize()
                    plan.close()
                    b.check_images(img, want, (layout, mapping, lanes, trials))
        b.check_pcm_untouched(pcm, (layout, "encode input"))
        if layout == "uniform" and ch <= 2:
            assert all(o % 64 == 0 for o in b.img_off) and img.data_ptr() % 64 == 0
            monkeypatch.setenv("AAD_HIP_ENCODE_RING", "2")  # read when a context is created
            ring = Engine(0)
            try:
                ring.set_mapping("dense")
                b.img_win.fill(img, IMG_CANARY)
                plan = ring.encode_plan(b.param(0), b.descs)
                plan.run(pcm, img)
                torch.cuda.synchronize()
                plan.close()
            finally:
                ring.close()
                monkeypatch.delenv("AAD_HIP_ENCODE_RING")
            b.check_images(img, [ob.encode(p, bits, 1024, 48000, ms, 0) for p in b.pcm], (layout, "dense byte ring"))
    del pcm, img


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("bits", [4, 3, 2])
def test_decode_plans(engine, bits, cfg):
    """AADHip_DecodePlanRun with every mapping - split decoder (quad, auto at this size), quad-fused, dense per-lane, sector-tiled
    (dense-tiled; mono / stereo, 16-byte-aligned PCM; 3-bit rows on the uniform layout's common code phase) - over the oracle's
    images placed across bytes 2^31 and 2^32, into a second PCM buffer at the streams' offsets across elements 2^31 and 2^32:
    the uniform branch (arithmetic-progression table) and the table branch.  The output buffer's canary must survive."""
    import torch
    from aad_amd.engine import parse_header
    _need(14)
    ch, ms = CONFIGS[cfg]
    rc, block_size, spb = ob.geometry(1024, ch, bits)
    assert rc == 0
    _, img, out = _plan_buffers(need_pcm=False)
    for layout in ("uniform", "table"):
        b = Batch(layout, bits, cfg, _plan_frames(layout, spb, 3), 4200 + 10 * bits + ch + ms, _encoded_size(engine, bits, cfg))
        images = [ob.encode(p, bits, 1024, 48000, ms, 0) for p in b.pcm]
        want = [ob.decode(w)[0] for w in images]
        b.img_win.fill(img, IMG_CANARY, [(o, np.frombuffer(w, dtype=np.uint8)) for o, w in zip(b.img_off, images)])
        header = parse_header(images[0][:31])
        for mapping in MAPPINGS:
            b.pcm_win.fill(out, OUT_CANARY)
            engine.set_mapping(mapping)
            plan = engine.decode_plan(header, b.descs, True)
            plan.run(img, out)
            torch.cuda.synchronize()
            plan.close()
            b.check_out(out, want, (layout, mapping))
        b.check_images(img, images, (layout, "decode input"))
    del img, out


def _reconstruct(engine, param, descs, pcm, img, out, kind, stats, seg=None):
    """one AADHip_ReconstructPlanCreate (or its segmented form) + AADHip_ReconstructPlanRun over a hand-made table"""
    import torch
    lib, plan = engine.lib, C.c_void_p()
    torch.cuda.synchronize()
    if seg is None:
        rc = lib.AADHip_ReconstructPlanCreate(engine._ctx, C.byref(param), len(descs), descs.ctypes.data, C.byref(plan))
    else:
        rc = lib.AADHip_SegmentedReconstructPlanCreate(engine._ctx, C.byref(param), C.byref(AADHipSegmentation(*seg)), len(descs),
                                                       descs.ctypes.data, C.byref(plan))
    assert rc == 0, ("reconstruct plan create", rc, engine.last_error())
    try:
        rc = lib.AADHip_ReconstructPlanRun(plan, pcm.data_ptr(), img.data_ptr(), out.data_ptr(), kind, stats.data_ptr())
        assert rc == 0, ("reconstruct plan run", rc, engine.last_error())
    finally:
        lib.AADHip_ReconstructPlanDestroy(plan)  # synchronises the context's stream
    torch.cuda.synchronize()


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("bits", [4, 3, 2])
def test_reconstruct_plans(engine, bits, cfg):
    """AADHip_ReconstructPlanRun (encode -> decode -> residual / statistics on the device) on both layouts, every mapping, decoded
    and residual output: the scratch images are the oracle's encode, the output is its decode or aado_residual, and the device
    statistics are ob.error_stats bit for bit under the sequential compare order."""
    import torch
    _need(23)
    ch, ms = CONFIGS[cfg]
    rc, block_size, spb = ob.geometry(1024, ch, bits)
    assert rc == 0
    engine.set_compare_order(sequential=True)
    pcm, img, out = _plan_buffers()
    stats = torch.empty((9, 3), dtype=torch.float64, device="cuda")
    for layout in ("uniform", "table"):
        b = Batch(layout, bits, cfg, _plan_frames(layout, spb, 2), 4300 + 10 * bits + ch + ms, _encoded_size(engine, bits, cfg))
        b.put_pcm(pcm)
        images = [ob.encode(p, bits, 1024, 48000, ms, 0) for p in b.pcm]
        decoded = [ob.decode(w)[0] for w in images]
        want_stats = [ob.error_stats(x, y) for x, y in zip(b.pcm, decoded)]
        for mapping in MAPPINGS:
            engine.set_mapping(mapping)
            for kind, want in ((RECONSTRUCT_DECODED, decoded), (RECONSTRUCT_RESIDUAL, [ob.residual(x, y) for x, y in zip(b.pcm, decoded)])):
                b.img_win.fill(img, IMG_CANARY)
                b.pcm_win.fill(out, OUT_CANARY)
                stats.fill_(-1.0)
                _reconstruct(engine, b.param(), b.descs, pcm, img, out, kind, stats)
                where = (layout, mapping, kind)
                b.check_images(img, images, where)
                b.check_out(out, want, where)
                got = [tuple(float(v) for v in r) for r in stats.cpu().numpy()]
                assert got == want_stats, where
        b.check_pcm_untouched(pcm, (layout, "reconstruct input"))
    del pcm, img, out


SEG_CASES = [(4, "stereo"), (3, "ms"), (2, "mono"), (4, "ch8")]


@pytest.mark.parametrize("bits,cfg", SEG_CASES)
@pytest.mark.parametrize("L,W", [(1, 0), (4, 2), (16, 3)])
def test_segmented_plans(engine, L, W, bits, cfg):
    """AADHip_SegmentedEncodePlanCreate (every mapping, trials 0 and 2) and AADHip_SegmentedReconstructPlanCreate (decoded and
    residual output, sequential statistics) on both placements - the chain records aim at virtual image starts in front of
    chains whose bytes lie across and beyond bytes 2^31 and 2^32, their PCM across and beyond elements 2^31 and 2^32 - against
    the segmented definition (tests/segment_oracle.py)."""
    import torch
    _need(23)
    ch, ms = CONFIGS[cfg]
    rc, block_size, spb = ob.geometry(1024, ch, bits)
    assert rc == 0
    engine.set_compare_order(sequential=True)
    pcm, img, out = _plan_buffers()
    stats = torch.empty((9, 3), dtype=torch.float64, device="cuda")
    for layout in ("uniform", "table"):
        b = Batch(layout, bits, cfg, _plan_frames(layout, spb, 40), 4400 + 100 * L + 10 * bits + ch + ms, _encoded_size(engine, bits, cfg))
        assert all(-(-n // spb) > 2 * L for n in b.frames)  # several chains per stream
        b.put_pcm(pcm)
        for trials in (0, 2):
            want = [so.segmented_encode(p, bits, L, W, 1024, ms=ms, trials=trials) for p in b.pcm]
            for mapping in MAPPINGS:
                b.img_win.fill(img, IMG_CANARY)
                engine.set_mapping(mapping)
                plan = engine.encode_plan(b.param(trials), b.descs, segment_blocks=L, warmup_blocks=W)
                plan.run(pcm, img)
                torch.cuda.synchronize()
                plan.close()
                b.check_images(img, want, (layout, mapping, trials))
        images = [so.segmented_encode(p, bits, L, W, 1024, ms=ms) for p in b.pcm]
        decoded = [ob.decode(w)[0] for w in images]
        want_stats = [ob.error_stats(x, y) for x, y in zip(b.pcm, decoded)]
        for mapping in ("auto", "dense", "quad"):
            engine.set_mapping(mapping)
            for kind, want in ((RECONSTRUCT_DECODED, decoded), (RECONSTRUCT_RESIDUAL, [ob.residual(x, y) for x, y in zip(b.pcm, decoded)])):
                b.img_win.fill(img, IMG_CANARY)
                b.pcm_win.fill(out, OUT_CANARY)
                stats.fill_(-1.0)
                _reconstruct(engine, b.param(), b.descs, pcm, img, out, kind, stats, seg=(L, W))
                where = (layout, "segmented reconstruct", mapping, kind)
                b.check_images(img, images, where)
                b.check_out(out, want, where)
                assert [tuple(float(v) for v in r) for r in stats.cpu().numpy()] == want_stats, where
        b.check_pcm_untouched(pcm, (layout, "segmented input"))
    del pcm, img, out


# ---- 2. host batches at the default wave budget ----------------------------------------------------------------------------------

HOST_FRAMES = 1 << 24  # stereo frames of each distinct host buffer (64 MiB)
HOST_STREAMS = 160     # prefixes of three buffers, every length different: ~8.8 GiB of PCM in one wave
_host_cache = {}


def host_buffer(k):
    """distinct host buffer k (int16 [HOST_FRAMES, 2]): white noise of a different level each"""
    rng = np.random.default_rng(9100 + k)
    amp = (1500, 9000, 30000)[k]
    return rng.integers(-amp, amp + 1, size=(HOST_FRAMES, 2), dtype=np.int16)


def host_batch():
    """(buffer, frames) per stream: neighbours come from different buffers, every length differs"""
    return [(i % 3, HOST_FRAMES - 1 - 25013 * ((37 * i) % HOST_STREAMS)) for i in range(HOST_STREAMS)]


_worker_buffer = [None, None]


def _oracle_job(job):
    """one stream of a host batch by the oracle (in a worker process): ("stats", k, n, bits, L, W) -> `aad -c`'s statistics of the
    serial encode (L None) or the segmented one; ("image", ...) -> sha256 of the segmented image"""
    kind, k, n, bits, L, W = job
    if _worker_buffer[0] != k:
        _worker_buffer[:] = [k, host_buffer(k)]
    x = _worker_buffer[1][:n]
    image = ob.encode(x, bits) if L is None else so.segmented_encode(x, bits, L, W)
    if kind == "image":
        return hashlib.sha256(image).hexdigest()
    return ob.error_stats(x, ob.decode(image)[0])


def _oracle(jobs):
    """the oracle's results of `jobs`, each distinct job computed once per session in a pool of at most 16 fresh processes"""
    import multiprocessing
    todo = sorted(set(j for j in jobs if j not in _host_cache), key=lambda j: (j[1], j[2]))
    if todo:
        workers = min(16, len(os.sched_getaffinity(0)), len(todo))
        with multiprocessing.get_context("spawn").Pool(workers) as pool:
            for j, r in zip(todo, pool.map(_oracle_job, todo, chunksize=4)):
                _host_cache[j] = r
    return [_host_cache[j] for j in jobs]


def _wave_rows(frames, ch):
    """the start of every stream's row in a wave's PCM block (int16 elements): rows one after the other, each rounded up to 8
    elements (aad_hip_engine.hip reconstruct_wave / aad_segments.h build_segment_waves: chains of a stream lie in order)"""
    rows = np.cumsum([0] + [_round_up(n * ch, 8) for n in frames])
    return rows[:-1], int(rows[-1])


def _assert_one_wave(engine, frames, ch, footprint):
    """the batch is one wave of the default budget (three quarters of the free memory) and its rows cross 2^31 and 2^32 elements"""
    import torch
    rows, total = _wave_rows(frames, ch)
    assert total > B32 + (1 << 28), total
    for x in (B31, B32):
        assert any(r < x < r + n * ch for r, n in zip(rows, frames)), ("no row across element", x)
    free, _ = torch.cuda.mem_get_info()
    assert footprint <= free // 4 * 3, ("the batch would not be one wave", footprint, free)


def _host_run(engine, segmentation, bits):
    from aad_amd.capi import ERROR_STATS_DTYPE
    param = make_parameter(2, bits, 1024, 48000, False, 0)
    batch = host_batch()
    bufs = [host_buffer(k) for k in range(3)]
    frames = [n for _, n in batch]
    footprint = sum(2 * _round_up(n * 2, 8) * 2 + _round_up(engine.encoded_size(param, n), 16) + 24 for n in frames)
    _assert_one_wave(engine, frames, 2, footprint)
    engine.set_tile_kbytes(0)
    engine.set_compare_order(sequential=True)
    n = len(batch)
    nsamp = np.array(frames, dtype=np.uint32)
    pp = (C.c_void_p * n)(*[bufs[k].ctypes.data for k, _ in batch])
    stats = np.zeros(n, dtype=ERROR_STATS_DTYPE)
    if segmentation is None:
        rc = engine.lib.AADHip_ReconstructBatch(engine._ctx, C.byref(param), n, pp, nsamp.ctypes.data, RECONSTRUCT_DECODED, None,
                                                stats.ctypes.data)
    else:
        rc = engine.lib.AADHip_SegmentedReconstructBatch(engine._ctx, C.byref(param), C.byref(AADHipSegmentation(*segmentation)), n, pp,
                                                         nsamp.ctypes.data, RECONSTRUCT_DECODED, None, stats.ctypes.data)
    assert rc == 0, (rc, engine.last_error())
    L, W = segmentation if segmentation is not None else (None, 0)
    want = _oracle([("stats", k, f, bits, L, W) for k, f in batch])
    got = [tuple(float(v) for v in s) for s in stats]
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, ("streams whose statistics differ", bad[:10], [(got[i], want[i]) for i in bad[:3]])


def test_reconstruct_batch(engine):
    """AADHip_ReconstructBatch, statistics only, stereo 4-bit, tile budget 0 (the real wave_budget()): one wave of 160 streams,
    ~4.7 * 10^9 PCM elements (~8.8 GiB) whose rows cross elements 2^31 and 2^32 (bytes 2^32 and 2^33) in the wave's PCM block,
    staged up through the pinned blocks; every stream's sequential statistics equal the oracle's."""
    _need(24)
    _host_run(engine, None, 4)


def test_segmented_reconstruct_batch(engine):
    """AADHip_SegmentedReconstructBatch (L = 64, W = 2), statistics only, stereo 3-bit, at the default wave budget: the same one
    wave of > 2^32 PCM elements; every stream's statistics equal those of the segmented definition's decode."""
    _need(24)
    _host_run(engine, (64, 2), 3)


def test_segmented_encode_batch(engine):
    """AADHip_SegmentedEncodeBatch (L = 64, W = 2), stereo 2-bit, at the default wave budget: one wave whose chains' PCM (staged to
    `row`) crosses elements 2^31 and 2^32 and whose ~1.1 GiB of images come back through `spot`; every image equals
    segment_oracle.segmented_encode (compared by sha256)."""
    import torch
    _need(20)
    bits, L, W = 2, 64, 2
    param = make_parameter(2, bits, 1024, 48000, False, 0)
    batch = host_batch()
    bufs = [host_buffer(k) for k in range(3)]
    frames = [f for _, f in batch]
    sizes = [engine.encoded_size(param, f) for f in frames]
    _assert_one_wave(engine, frames, 2, sum(_round_up(f * 2, 8) * 2 + _round_up(s, 16) for f, s in zip(frames, sizes)))
    engine.set_tile_kbytes(0)
    n = len(batch)
    outs = [np.zeros(s, dtype=np.uint8) for s in sizes]
    got_sizes = np.zeros(n, dtype=np.uint64)
    caps = np.array(sizes, dtype=np.uint64)
    nsamp = np.array(frames, dtype=np.uint32)
    pp = (C.c_void_p * n)(*[bufs[k].ctypes.data for k, _ in batch])
    op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    rc = engine.lib.AADHip_SegmentedEncodeBatch(engine._ctx, C.byref(param), C.byref(AADHipSegmentation(L, W)), n, pp, nsamp.ctypes.data,
                                                op, caps.ctypes.data, got_sizes.ctypes.data)
    assert rc == 0, (rc, engine.last_error())
    assert [int(s) for s in got_sizes] == sizes
    got = [hashlib.sha256(o).hexdigest() for o in outs]
    del outs
    want = _oracle([("image", k, f, bits, L, W) for k, f in batch])
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, ("streams whose image differs", bad[:10])
    torch.cuda.synchronize()


# ---- 3. one stream larger than 4 GiB ---------------------------------------------------------------------------------------------

def test_one_stream_past_4gib(engine):
    """One stereo 4-bit stream of 2^32 - 1 frames: 16 GiB of PCM (in-stream offsets first * ch up to 2^33 elements) and a 4.1 GiB
    image (block offsets header + b * block_size past 2^31 and 2^32 bytes).  Segmented plan with L = 1, W = 0 - each block a fresh
    encoder over its own frames (include/aad_hip.h), so every all-zero block has the same bytes and a marked block is ob.encode of
    its frames without the file header.  The PCM is zero apart from marked blocks (noise) on either side of elements 2^31 and 2^32
    and of image bytes 2^31 and 2^32, block 0 and the short last block.  A serial (unsegmented) encode of this stream is one chain
    of 4.3 million blocks per channel and out of scope.
    The image is then decoded with every mapping (auto and dense-tiled: the sector-tiled decoder; dense: per-lane with streamed
    stores; quad and quad-fused: the fused quad decoder - the split decoder's residual scratch would exceed its cap), as a
    one-stream plan (uniform branch) and as a two-stream table (table branch; the second stream decodes block 0 again into the
    tail of the buffer); each block decodes from its own header.  Blocks are compared on the device against the zero block's
    decode; only marked blocks come to the host."""
    import torch
    from aad_amd.engine import parse_header
    _need(22)
    ch, bits = 2, 4
    N = B32 - 1
    rc, block_size, spb = ob.geometry(1024, ch, bits)
    assert rc == 0 and block_size == 1024
    param = make_parameter(ch, bits, 1024, 48000, False, 0)
    blocks = -(-N // spb)
    size = engine.encoded_size(param, N)
    last = N - (blocks - 1) * spb  # frames of the short last block
    assert 0 < last < spb and N * ch * 2 > B33 and size > B32

    marks = {0, blocks - 1}
    for x in (B31, B32):  # PCM elements (bytes 2^32, 2^33)
        b = x // ch // spb
        assert b * spb * ch < x < (b + 1) * spb * ch
        marks |= {b - 1, b, b + 1}
    for x in (B31, B32):  # image bytes
        b = (x - 31) // block_size
        assert 31 + b * block_size < x < 31 + (b + 1) * block_size
        marks |= {b - 1, b, b + 1}
    marks = sorted(marks)
    frames_of = lambda b: last if b == blocks - 1 else spb
    marked = {b: _synth(7000 + b, frames_of(b), ch, 1) for b in marks}

    zero_img = ob.encode(np.zeros((spb, ch), dtype=np.int16), bits)
    assert len(zero_img) == 31 + block_size
    zero_block, zero_dec = zero_img[31:], ob.decode(zero_img)[0].reshape(-1)
    head = bytearray(zero_img[:31])
    head[14:18] = N.to_bytes(4, "big")
    want_block = {b: ob.encode(x, bits)[31:] for b, x in marked.items()}
    want_dec = {b: ob.decode(ob.encode(x, bits))[0].reshape(-1) for b, x in marked.items()}
    assert all(want_block[b] != zero_block for b in marks if b != blocks - 1)
    assert len(want_block[blocks - 1]) == size - 31 - (blocks - 1) * block_size

    # encode
    pcm = torch.zeros(N * ch, dtype=torch.int16, device="cuda")
    for b, x in marked.items():
        pcm[b * spb * ch:b * spb * ch + x.size].copy_(torch.from_numpy(x.reshape(-1)))
    img = torch.full((size + MARGIN,), IMG_CANARY, dtype=torch.uint8, device="cuda")
    d = np.zeros(1, dtype=STREAM_DESC_DTYPE)
    d["data_size"], d["num_samples"] = size, N
    plan = engine.encode_plan(param, d, segment_blocks=1, warmup_blocks=0)
    plan.run(pcm, img)
    torch.cuda.synchronize()
    plan.close()
    del pcm
    torch.cuda.empty_cache()

    def differing(rows, row):
        """indices of the rows of a 2-D device tensor that differ from `row`, in chunks of 256 MiB"""
        step = max(1, (1 << 28) // (rows.shape[1] * rows.element_size()))
        found = []
        for lo in range(0, rows.shape[0], step):
            found += (torch.nonzero((rows[lo:lo + step] != row).any(dim=1)).flatten() + lo).tolist()
        return found

    assert bytes(img[:31].cpu().numpy()) == bytes(head)
    body = img[31:31 + (blocks - 1) * block_size].view(blocks - 1, block_size)
    full_marks = [b for b in marks if b != blocks - 1]
    assert differing(body, torch.from_numpy(np.frombuffer(zero_block, dtype=np.uint8).copy()).cuda()) == full_marks
    for b in marks:
        got = bytes(img[31 + b * block_size:min(31 + (b + 1) * block_size, size)].cpu().numpy())
        assert got == want_block[b], ("encoded block", b)
    assert bool((img[size:] == IMG_CANARY).all())

    # decode: uniform branch (one stream) and table branch (a second stream decodes block 0 into the tail)
    header = parse_header(bytes(head))
    tail = _round_up(N * ch + MARGIN, 8)
    out = torch.empty(tail + spb * ch + MARGIN, dtype=torch.int16, device="cuda")
    zero_row = torch.from_numpy(zero_dec.copy()).cuda()
    one = np.zeros(1, dtype=STREAM_DESC_DTYPE)
    one["data_size"], one["num_samples"] = size, N
    two = np.zeros(2, dtype=STREAM_DESC_DTYPE)
    two[0] = one[0]
    two["pcm_offset"][1], two["data_size"][1], two["num_samples"][1] = tail, 31 + block_size, spb
    for mapping in MAPPINGS:
        for descs in (one, two):
            out.fill_(OUT_CANARY)
            engine.set_mapping(mapping)
            plan = engine.decode_plan(header, descs, True)
            plan.run(img, out)
            torch.cuda.synchronize()
            plan.close()
            where = (mapping, len(descs))
            rows = out[:(blocks - 1) * spb * ch].view(blocks - 1, spb * ch)
            assert differing(rows, zero_row) == full_marks, where
            for b in marks:
                got = out[b * spb * ch:b * spb * ch + frames_of(b) * ch].cpu().numpy()
                assert np.array_equal(got, want_dec[b]), where + ("decoded block", b)
            rest = out[N * ch:]
            if len(descs) == 2:
                assert np.array_equal(out[tail:tail + spb * ch].cpu().numpy(), want_dec[0]), where
                rest = torch.cat([out[N * ch:tail], out[tail + spb * ch:]])
            assert bool((rest == OUT_CANARY).all()), where
    del img, out, body, rows, zero_row
