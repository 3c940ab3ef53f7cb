"""Level statistics of reverberated rows (AADHip_ConvolverRunStats, include/aad_hip.h "reverberation") restated in numpy: v comes
from convolve_oracle.to_int16 over the oracle's exact sums, the sums of a record are Python integers, `count` is the closed form
of aad_convolve.h's convolve_output_count beside a brute force over the stream's length.  The mistakes a kernel can make are here
as well, as mutants of the record, so that a test can assert on the CPU that its inputs catch each of them.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import numpy as np

import convolve_oracle as co
import window_placed_oracle as po

U64 = 1 << 64
TILE, BLOCK, WAVES = 4096, 256, 4  # aad_convolve.h: a workgroup's tile, an accumulator tile, the waves that share a tile's blocks


def output_count(c_src, source_frames, shift, le):
    """the closed form of aad_convolve.h's convolve_output_count"""
    c = min(int(c_src), int(source_frames))
    if c <= shift:
        return 0
    return min(int(le), c - shift)


def output_count_brute(c_src, source_frames, shift, le):
    c = min(int(c_src), int(source_frames))
    return sum(1 for n in range(int(le)) if shift + n < c)


def record(v, count):
    """v: the integer values of one row's first Le frames -> [sum_sq, sum_abs, max_abs, count], Python integers"""
    v = [abs(int(x)) for x in v]
    return [sum(x * x for x in v), sum(v), max(v, default=0), int(count)]


def values(acc, q, clamp=True):
    """the int16 element of every sum; clamp=False: the mutant that takes the record from the unclamped value"""
    if clamp:
        return co.to_int16(acc, q).astype(np.int64)
    acc = np.asarray(acc, dtype=np.int64)
    return (acc + (1 << (q - 1) if q else 0)) >> q


def expected_stats(acc, qs, spans, counts, has_response=None, clamp=True, over_row=False):
    """acc: int64 [N, C, T], qs: [N], counts: [N] or [N, C] -> int64 [N, C, 4] over each window's first Le frames; a window without
    a response: zeros.  clamp=False (Python integers in an object array: an unclamped v^2 reaches 2^90), over_row=True (sums over T
    instead of Le): mutants."""
    n, ch, frames = acc.shape
    counts = np.asarray(counts, dtype=np.int64).reshape(n, -1)
    out = np.zeros((n, ch, 4), dtype=np.int64 if clamp else object)
    for w, (le, _) in enumerate(po.clipped(spans, n, frames)):
        if has_response is not None and not has_response[w]:
            continue
        for c in range(ch):
            v = values(acc[w, c], int(qs[w]), clamp)
            out[w, c] = record(v if over_row else v[:le], counts[w, c % counts.shape[1]])
    return out


def stream_counts(lengths, windows, index, responses, frames, spans, ignore_shift=False):
    """int64 [N]: per window the closed form over the source batch's count - window decode's count of the source window that
    AADHip_ConvolverResolve writes - held against the brute force #{n < Le : first_frame + n < num_samples[stream]}; 0 without a
    response.  ignore_shift=True: the mutant whose count forgets the lane's shift (no brute force then)."""
    windows = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
    t_src = co.source_frames(frames, responses)
    out = np.zeros(len(windows), dtype=np.int64)
    for w, ((s, first), (le, _)) in enumerate(zip(windows.tolist(), po.clipped(spans, len(windows), frames))):
        r = (0 if index is None else int(index[w])) % U64
        s, first = s % U64, first % U64
        if r >= len(responses):
            continue
        _, src_first, _, shift = co.resolve(s, first, r, responses)
        length = int(lengths[s]) if s < len(lengths) else 0
        c_src = min(max(length - src_first, 0), t_src)  # the frames of the source window the stream had
        if ignore_shift:
            out[w] = output_count(c_src, t_src, 0, le)
            continue
        closed = output_count(c_src, t_src, shift, le)
        brute = sum(1 for n in range(le) if first + n < length)
        assert closed == brute == output_count_brute(c_src, t_src, shift, le), (w, s, first, closed, brute)
        out[w] = closed
    return out


def wave_partials(v, n0, n_end):
    """the kernel's tile: blocks of 256 outputs, block b kept by wave b % 4 -> per wave [sum_sq, sum_abs, max_abs] of v[n0:n_end]"""
    parts = [[0, 0, 0] for _ in range(WAVES)]
    for b, lo in enumerate(range(n0, n_end, BLOCK)):
        r = record(v[lo:min(lo + BLOCK, n_end)], 0)
        p = parts[b % WAVES]
        p[0], p[1], p[2] = p[0] + r[0], p[1] + r[1], max(p[2], r[2])
    return parts


def stale_scratch_stats(acc, qs, spans, counts):
    """the mutant whose idle waves leave their slot of the scratch alone: a wave without a block in a tile adds what the slot held
    from the tile before it (the row's previous tile, as a workgroup that walks a row would leave it) once more.  A model for the
    CPU: it shows that the inputs have idle waves beside loud slots, so a kept slot WOULD change a record.  On the device a
    workgroup's items lie 2^20 apart and never walk a row; a wave that failed to write its slot would leave whatever the LDS held,
    which the T = 257 and T = 4360 cases catch only where that is not zero.  The case that does run two items through one
    scratch is the item loop's (tests/convolve_stats_cases.py, item_loop_rows)."""
    n, ch, frames = acc.shape
    out = expected_stats(acc, qs, spans, counts)
    for w, (le, _) in enumerate(po.clipped(spans, n, frames)):
        for c in range(ch):
            v = values(acc[w, c], int(qs[w]))
            slots = [[0, 0, 0] for _ in range(WAVES)]
            for n0 in range(0, le, TILE):
                n_end = min(n0 + TILE, le)
                blocks = -(-(n_end - n0) // BLOCK)
                parts = wave_partials(v, n0, n_end)
                for wave in range(WAVES):
                    if wave < blocks:
                        slots[wave] = parts[wave]
                    else:  # idle: the stale slot is counted again
                        out[w, c, 0] += slots[wave][0]
                        out[w, c, 1] += slots[wave][1]
                        out[w, c, 2] = max(out[w, c, 2], slots[wave][2])
    return out
