"""The hand-made inputs of tests/test_gpu_convolve_stats.py, in numpy alone: tests/test_convolve_stats_host.py asserts on the CPU
that each of them catches the mistake it is there for (the mutants of tests/convolve_stats_oracle.py) before the GPU file runs
them.  The responses are the oracle's quantisation of the float taps; the GPU file holds the library's own to it.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
from collections import namedtuple

import numpy as np

import convolve_oracle as co
import convolve_stats_oracle as so
import window_placed_oracle as po

Case = namedtuple("Case", "frames floats delays responses rows lanes c_src acc qs has_response span_sets")


def _quantised(floats, delays):
    out = []
    for h, d in zip(floats, delays):
        taps, q, delay = co.quantise(h, d)
        out.append((taps.astype(np.int64), q, delay))
    return out


def _acc(rows, lanes, frames, responses):
    """int64 acc [N, C, frames] and q per window; a lane without a response: zeros"""
    acc = np.zeros(rows.shape[:2] + (frames,), dtype=np.int64)
    qs = np.zeros(len(rows), dtype=np.int64)
    has = np.zeros(len(rows), dtype=bool)
    for w in range(len(rows)):
        r = int(lanes[w, 0]) & 0xFFFFFFFF
        if r >= len(responses):
            continue
        taps, qs[w], d = responses[r]
        has[w] = True
        for c in range(rows.shape[1]):
            acc[w, c] = co.sums(rows[w, c], int(lanes[w, 1]), frames, taps, d)
    return acc, qs, has


def counts_of(case, spans, ignore_shift=False):
    """int64 [N, C]: the closed form per row over the case's source counts"""
    n, ch = case.c_src.shape
    t_src = case.rows.shape[2]
    out = np.zeros((n, ch), dtype=np.int64)
    for w, (le, _) in enumerate(po.clipped(spans, n, case.frames)):
        if not case.has_response[w]:
            continue
        shift = 0 if ignore_shift else int(case.lanes[w, 1])
        for c in range(ch):
            out[w, c] = so.output_count(int(case.c_src[w, c]), t_src, shift, le)
            if not ignore_shift:
                assert out[w, c] == so.output_count_brute(int(case.c_src[w, c]), t_src, shift, le)
    return out


def tile_case():
    """T = 4360: a tile of 4096 outputs and one of two blocks (256 + 8 outputs) - waves 2 and 3 have no block there - with two
    channel rows a window; responses of 40 and 4200 taps (two staged pieces) and the unit response."""
    frames = 4096 + 264
    rng = np.random.default_rng(4360)
    floats = [rng.uniform(-0.9, 0.9, size=40), rng.uniform(-0.9, 0.9, size=4200) * np.exp(-np.arange(4200) * (6.0 / 4200)), np.ones(1)]
    floats[0][3], floats[1][1400] = 1.0, 1.0
    delays = [None, None, None]
    responses = _quantised(floats, delays)
    assert [(len(t), q, d) for t, q, d in responses] == [(40, 14, 3), (4200, 14, 1400), (1, 14, 0)]
    t_src = frames + 4199
    n, ch = 8, 2
    rows = rng.integers(-32768, 32768, size=(n, ch, t_src)).astype(np.int16)
    lead = [len(t) - 1 - d for t, _, d in responses]
    lanes = np.array([[0, lead[0]], [1, lead[1]], [2, 0], [0, lead[0]], [0xFFFFFFFF, 0], [1, 0], [0, 5], [2, 77]], dtype=np.uint32).view(np.int32)
    rows[2] = -32768                                       # the rail throughout: sum_sq = 4360 * 2^30
    rows[3, :, lead[0] + 4096 - 36:] = 0                   # the second tile reads zeros alone: no atomics there
    rows[3, 1, :lead[0] + 4096 - 36:7] = 0
    rows[7, 0] = np.where(np.arange(t_src) % 2 == 1, 32767, -32768)
    c_src = np.empty((n, ch), dtype=np.int64)
    c_src[:, 0] = [t_src, t_src, 3000, lead[0] + 4100, 500, 0, 5, t_src + 9]     # the whole row, a part, at the shift, past the row
    c_src[:, 1] = [lead[0] + 1, lead[1] - 1, 4361, 1 << 40, 7, 4360, 6, 78]
    acc, qs, has = _acc(rows, lanes, frames, responses)
    T = frames
    span_sets = [None,
                 np.array([(4200, 0), (0, 0), (10, T), (3000, 5), (T, 100), (4097, 263), (T, 0), (1 << 40, 4095)], dtype=np.int64),
                 np.array([(3000, 5), (4200, 0), (4097, 0), (T, 0), (T, 0), (10, T + 5), (0, 17), (4096, 0)], dtype=np.int64)]
    return Case(frames, floats, delays, responses, rows, lanes, c_src, acc, qs, has, span_sets)


ITEM_ROWS = (1 << 20) + 77  # a grid of 2^20 workgroups: the first 77 run a second item through the same scratch
ITEM_TAPS = 40


def item_loop_rows():
    """-> (float taps [40], int16 rows [2^20 + 77, 1, 40], c_src [N]): T = 1, lane (0, 0), delay K - 1 - the one output of a row
    reads all its 40 source frames"""
    rng = np.random.default_rng(2077)
    h = rng.uniform(-0.9, 0.9, size=ITEM_TAPS)
    h[0] = 1.0
    rows = rng.integers(-32768, 32768, size=(ITEM_ROWS, 1, ITEM_TAPS)).astype(np.int16)
    rows[100], rows[(1 << 20) + 9] = 0, 0  # silent rows: no atomics, the record still right - the second behind a loud first item
    c_src = (np.arange(ITEM_ROWS) % 3).astype(np.int64)  # count = min(1, c_src)
    return h, rows, c_src


def item_loop_expected(h, rows, c_src):
    """-> (int64 records [N, 1, 4], int64 v [N]); vectorised, held against the oracle's Python sums on a sample by the host test"""
    taps, q, d = co.quantise(h, ITEM_TAPS - 1)
    acc = rows[:, 0, ::-1].astype(np.int64) @ taps.astype(np.int64)  # sum_k h[k] x[K - 1 - k]
    v = co.to_int16(acc, q).astype(np.int64)
    u = np.abs(v)
    return np.stack([u * u, u, u, np.minimum(c_src, 1)], axis=1)[:, None, :], v
