"""GPU tests of the reconstruction modes: encode -> decode ->
residual / RMSE-MSD-MaxAE on the device, against the goldens made from the compiled reference CLI
(tests/golden/cli_modes.json, `aad -r` / `aad -g` / `aad -c`, src/main.c:275-503) and the oracle.

Bar: reconstructed and residual PCM bit-exact.  The three statistics are fp64 sums whose ORDER
differs from the CLI's channel-major walk by default (fixed reduction tree on the device), so they are held
to 1e-12 relative - and to the exact text of the line the CLI printed (six decimals), which the device
guarantees by taking the reference's order itself whenever the tree's result lies within the reordering bound
of a rounding boundary (aad_compare.hip.h); forced, that order gives the oracle's doubles bit for bit.  Streams that lie on
such a boundary (tests/golden/stats_ties.json) take that path by themselves and must give the reference's doubles bit for
bit, for both output kinds; the tree order is held to the exact statistics within the proven reordering bound."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from aad_amd.capi import make_parameter
from aad_amd.synth import synth_pcm
from helpers import (GOLDEN, cli_mode_input, exact_squares, exact_sum, reorder_bound, sha256, stats_tie_cases, stats_tie_input,
                     wav16_bytes)

pytestmark = pytest.mark.gpu
STATS_RTOL = 1e-12
CASES = json.load(open(os.path.join(GOLDEN, "cli_modes.json")))["cases"]
CLI = os.path.join(os.path.dirname(GOLDEN), "..", "aad_amd", "aad_batch")


@pytest.fixture(scope="module")
def engine():
    import torch  # noqa: F401
    from aad_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def test_statistics_in_the_reference_order_are_bit_identical(engine):
    """AAD_HIP_OPTION_COMPARE_ORDER = sequential: one lane per stream walks the values channel by channel, sample by
    sample, with separately rounded multiplies and adds - the reference's loop (src/main.c:478-497).  The three
    doubles must EQUAL the oracle's (==, not a tolerance): this is the path the device takes by itself whenever its
    tree sum lies close enough to a rounding boundary of the printed six decimals for the order to show, so the
    printed line is the reference's by construction.  Mono, stereo, 8 channels, lengths from one sample to several
    blocks, loud noise (large sums) and near-silence (tiny sums); decoded and residual output alike."""
    engine.set_compare_order(sequential=True)
    try:
        rng = np.random.default_rng(31)
        for ch, bits, trials, ms in ((1, 4, 0, False), (2, 4, 2, False), (2, 3, 0, True), (2, 2, 1, False), (8, 3, 0, False)):
            lengths = [1, 3, 4, 5, 17, 992, 993, 2500, int(rng.integers(3000, 9000))]
            pcms = [synth_pcm(1, n, ch, seed=500 + n, kind=["music", "noise", "nyquist"][k % 3])[0] for k, n in enumerate(lengths)]
            pcms.append((synth_pcm(1, 4000, ch, seed=9)[0] // 4096).astype(np.int16))  # a few LSBs of signal
            param = make_parameter(ch, bits, 1024, 48000, ms, trials)
            rec, stats = engine.reconstruct_host(pcms, param, residual=False)
            gap, stats_g = engine.reconstruct_host(pcms, param, residual=True)  # the walk reads the residual the segments kernel wrote
            for i, pcm in enumerate(pcms):
                want = ob.error_stats(pcm, rec[i])
                assert _as_tuple(stats[i]) == want, (ch, bits, trials, ms, len(pcm), _as_tuple(stats[i]), want)
                assert _as_tuple(stats_g[i]) == want, (ch, bits, trials, ms, len(pcm), _as_tuple(stats_g[i]), want)
                assert np.array_equal(gap[i], ob.residual(pcm, rec[i]))
    finally:
        engine.set_compare_order(sequential=False)
    # and the default order prints the same line for the same inputs
    for ch, bits in ((1, 4), (2, 2)):
        pcms = [synth_pcm(1, n, ch, seed=600 + n)[0] for n in (5, 992, 4001)]
        param = make_parameter(ch, bits, 1024, 48000, False, 0)
        rec, stats = engine.reconstruct_host(pcms, param, residual=False)
        for i, pcm in enumerate(pcms):
            assert ob.stats_line(_as_tuple(stats[i])) == ob.stats_line(ob.error_stats(pcm, rec[i]))


def _as_tuple(rec):
    return float(rec["rms_error"]), float(rec["mean_abs_error"]), float(rec["max_abs_error"])


def test_reconstruct_batch_matches_reference_cli(engine):
    """every golden case through AADHip_ReconstructBatch, grouped per parameter set so that mono and
    stereo inputs of different lengths share one call"""
    groups = {}
    for c in CASES:
        pcm, rate, _ = cli_mode_input(c)
        groups.setdefault((pcm.shape[1], rate, c["bits"], c["trials"], c["ms"]), []).append((c, pcm))
    assert len(groups) >= 12
    for (ch, rate, bits, trials, ms), members in groups.items():
        param = make_parameter(ch, bits, 1024, rate, ms, trials)
        pcms = [m[1] for m in members]
        rec, stats = engine.reconstruct_host(pcms, param, residual=False)
        gap, stats2 = engine.reconstruct_host(pcms, param, residual=True)
        only_stats = engine.reconstruct_host(pcms, param, want_pcm=False)[1]
        for i, (c, pcm) in enumerate(members):
            assert sha256(wav16_bytes(rec[i], rate)) == c["reconstructed_sha256"], c
            assert sha256(wav16_bytes(gap[i], rate)) == c["residual_sha256"], c
            assert ob.stats_line(_as_tuple(stats[i])) == c["stats_line"], c
            want = ob.error_stats(pcm, rec[i])
            np.testing.assert_allclose(_as_tuple(stats[i]), want, rtol=STATS_RTOL, atol=0)
            assert _as_tuple(stats[i])[2] == want[2]  # a maximum does not depend on the order
            assert _as_tuple(stats2[i]) == _as_tuple(stats[i]) == _as_tuple(only_stats[i])


@pytest.mark.parametrize("tile_kbytes", [1, 7, 300])
def test_reconstruct_batch_in_chunks_and_waves(engine, tile_kbytes):
    """AADHip_ReconstructBatch stages its PCM through the pinned blocks in chunks of the tile budget and, when the batch does
    not fit the device, runs it as several waves of whole streams (aad_hip_engine.hip, reconstruct_wave): a forced tile size
    (AAD_HIP_OPTION_TILE_KBYTES) makes the chunks a few KiB and the waves 64 tiles' worth, so that ragged batches - one-sample
    streams next to streams longer than a chunk AND longer than a wave, 1 / 2 / 8 channels, trial search, M/S - cross every
    boundary: chunk edges inside a stream's row, rows inside the padding between streams, the statistics block split over
    chunks.  Same bytes and the same doubles as the call with everything in one piece; PCM and the printed line == the oracle."""
    rng = np.random.default_rng(900 + tile_kbytes)
    for ch, bits, trials, ms, count in ((2, 4, 2, False, 90), (1, 3, 0, False, 400), (8, 2, 0, False, 40), (2, 2, 1, True, 130)):
        lengths = [int(rng.choice([1, 3, 4, 5, 200, 992, 993, int(rng.integers(1, 5000)), int(rng.integers(5000, 40000))])) for _ in range(count)]
        lengths[count // 2] = 150000  # longer than any wave at tile_kbytes = 1 (64 KiB): a wave of its own
        pcms = [synth_pcm(1, n, ch, seed=int(rng.integers(0, 1 << 30)), kind=str(rng.choice(["music", "noise"])))[0] for n in lengths]
        param = make_parameter(ch, bits, 1024, 48000, ms, trials)
        engine.set_tile_kbytes(0)
        rec0, stats0 = engine.reconstruct_host(pcms, param, residual=False)
        gap0, _ = engine.reconstruct_host(pcms, param, residual=True)
        engine.set_tile_kbytes(tile_kbytes)
        try:
            rec, stats = engine.reconstruct_host(pcms, param, residual=False)
            gap, stats_g = engine.reconstruct_host(pcms, param, residual=True)
            only = engine.reconstruct_host(pcms, param, want_pcm=False)[1]
            no_stats = engine.reconstruct_host(pcms, param, want_stats=False)[0]
        finally:
            engine.set_tile_kbytes(0)
        for i, pcm in enumerate(pcms):
            assert np.array_equal(rec[i], rec0[i]) and np.array_equal(gap[i], gap0[i]) and np.array_equal(no_stats[i], rec0[i]), (tile_kbytes, ch, bits, i, lengths[i])
            assert _as_tuple(stats[i]) == _as_tuple(stats0[i]) == _as_tuple(stats_g[i]) == _as_tuple(only[i]), (tile_kbytes, ch, bits, i, lengths[i])
        for i in list(range(0, count, 9)) + [count // 2]:
            want = ob.decode(ob.encode(pcms[i], bits, 1024, 48000, ms, trials))[0]
            assert np.array_equal(rec[i], want) and np.array_equal(gap[i], ob.residual(pcms[i], want)), (tile_kbytes, ch, bits, i, lengths[i])
            assert ob.stats_line(_as_tuple(stats[i])) == ob.stats_line(ob.error_stats(pcms[i], want))


@pytest.mark.parametrize("streams,samples,ch,bits", [(1000, 992, 2, 4), (3, 70001, 1, 3), (64, 4000, 8, 2)])
def test_reconstruct_device_resident_vs_oracle(engine, streams, samples, ch, bits):
    """device-resident form (AADHip_ReconstructPlanRun): nothing but the statistics needs to leave
    HBM; checked against oracle encode -> decode -> residual / statistics on sampled streams,
    including the 8-channel container extension and streams longer than one compare segment"""
    import torch
    pcm = synth_pcm(streams, samples, ch, seed=99)
    param = make_parameter(ch, bits, 1024, 48000, False, 0)
    d_pcm = torch.from_numpy(pcm).cuda()
    rec, stats = engine.reconstruct_uniform(d_pcm, param, residual=False)
    gap, stats_g = engine.reconstruct_uniform(d_pcm, param, residual=True)
    torch.cuda.synchronize()
    rec, gap, stats, stats_g = rec.cpu().numpy(), gap.cpu().numpy(), stats.cpu().numpy(), stats_g.cpu().numpy()
    assert np.array_equal(stats, stats_g)
    for s in range(0, streams, max(1, streams // 7)):
        want = ob.decode(ob.encode(pcm[s], bits, 1024))[0]
        assert np.array_equal(rec[s], want), s
        assert np.array_equal(gap[s], ob.residual(pcm[s], want)), s
        np.testing.assert_allclose(stats[s], ob.error_stats(pcm[s], want), rtol=STATS_RTOL, atol=0)
        assert stats[s][2] == ob.error_stats(pcm[s], want)[2]


def test_reconstruct_wraparound_corner(engine):
    """|x - y| >= 32768 cannot come out of the codec for real input, but the residual's int16 wrap
    and the statistics' 32-bit wrap (src/main.c:419-423, 470-474) are part of what the CLI does:
    a full-scale square wave at 2 bits drives the reconstruction far enough off to exercise large
    differences; the oracle restates the same wraps"""
    n = 3000
    x = np.where((np.arange(n) // 3) % 2 == 0, 32767, -32768).astype(np.int16).reshape(-1, 1)
    param = make_parameter(1, 2, 1024, 48000, False, 0)
    rec, stats = engine.reconstruct_host([x], param)
    gap, _ = engine.reconstruct_host([x], param, residual=True)
    want = ob.decode(ob.encode(x, 2, 1024))[0]
    assert np.array_equal(rec[0], want)
    assert np.array_equal(gap[0], ob.residual(x, want))
    np.testing.assert_allclose(_as_tuple(stats[0]), ob.error_stats(x, want), rtol=STATS_RTOL, atol=0)
    assert _as_tuple(stats[0])[2] == ob.error_stats(x, want)[2]


CANARY = 0x3C5A  # int16 written between the streams of a hand-made plan: no kernel may touch it


def _plan_run(engine, param, pcms, residual, rng):
    """pcms (int16 [frames, channels] each) as ONE AADHip_ReconstructPlanCreate / AADHip_ReconstructPlanRun over a hand-made
    stream table: rows out of order, odd gaps of canary values between them and around them, images out of order too.
    -> (output rows, stats float64 [streams, 3]); every canary of the output buffer is checked."""
    import ctypes as C
    import torch
    from aad_amd.capi import STREAM_DESC_DTYPE
    from aad_amd.engine import RECONSTRUCT_DECODED, RECONSTRUCT_RESIDUAL, _check
    n = len(pcms)
    order = rng.permutation(n)
    d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
    pos, data = int(rng.integers(1, 40)), 0
    for i in order:
        size = engine.encoded_size(param, pcms[i].shape[0])
        d["pcm_offset"][i], d["data_offset"][i], d["data_size"][i], d["num_samples"][i] = pos, data, size, pcms[i].shape[0]
        pos += pcms[i].size + int(rng.integers(1, 40))
        data += -(-size // 16) * 16 + 16
    pos += 64  # canaries behind the last row too
    host_in = rng.integers(-32768, 32768, pos).astype(np.int16)  # junk in the gaps: never read
    row = np.zeros(pos, dtype=bool)
    for i in range(n):
        o = int(d[i]["pcm_offset"])
        host_in[o:o + pcms[i].size] = pcms[i].reshape(-1)
        row[o:o + pcms[i].size] = True
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((pos,), CANARY, dtype=torch.int16, device="cuda")
    images = torch.empty(data, dtype=torch.uint8, device="cuda")
    stats = torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    plan = C.c_void_p()
    _check("AADHip_ReconstructPlanCreate", engine.lib.AADHip_ReconstructPlanCreate(engine._ctx, C.byref(param), n, d.ctypes.data, C.byref(plan)))
    try:
        cur = engine._enter()
        _check("AADHip_ReconstructPlanRun", engine.lib.AADHip_ReconstructPlanRun(
            plan, d_in.data_ptr(), images.data_ptr(), d_out.data_ptr(), RECONSTRUCT_RESIDUAL if residual else RECONSTRUCT_DECODED,
            stats.data_ptr()))
        engine._exit(cur)
    finally:
        engine.lib.AADHip_ReconstructPlanDestroy(plan)  # synchronises the stream first
    out = d_out.cpu().numpy()
    assert np.all(out[~row] == CANARY), np.nonzero(out[~row] != CANARY)[0][:8]
    rows = [out[int(d[i]["pcm_offset"]):int(d[i]["pcm_offset"]) + pcms[i].size].reshape(pcms[i].shape) for i in range(n)]
    return rows, stats.cpu().numpy()


def _tie_groups():
    groups = {}
    for c in stats_tie_cases():
        groups.setdefault((c["channels"], c["bits"], c["block_size"], c["ms"], c["trials"]), []).append(c)
    return sorted(groups.items())


@pytest.mark.parametrize("key,cases", [pytest.param(k, v, id="c%d_b%d_ms%d" % (k[0], k[1], k[3])) for k, v in _tie_groups()])
def test_statistics_at_rounding_ties(engine, key, cases):
    """tests/golden/stats_ties.json: streams whose RMSE or MSD lies within a quarter of compare_finish_kernel's window of a
    rounding boundary of the printed six decimals, so that the device must re-sum them in the reference's order - and controls
    just outside the window, which it must not.  Under the DEFAULT order (the tree), through AADHip_ReconstructBatch with decoded
    and residual output, with and without the PCM returned, in one piece and in 1 KiB tiles (every stream a wave of its own), and
    through a hand-made ReconstructPlanRun that mixes them into a ragged batch of other streams: the tie cases' three doubles
    EQUAL the reference's (bitwise: a tree sum of 10^5 or more terms differs from them in the last bits) and every line is the
    reference CLI's.  The residual kinds failed before the re-sum learnt to read the residual (it was skipped there)."""
    ch, bits, block, ms, trials = key
    param = make_parameter(ch, bits, block, 48000, ms, trials)
    pcms = [stats_tie_input(c) for c in cases]
    want = [tuple(float.fromhex(h) for h in c["stats_hex"]) for c in cases]
    rec0 = None
    for tile in (0, 1):
        engine.set_tile_kbytes(tile)
        try:
            for residual in (False, True):
                for want_pcm in (True, False):
                    out, stats = engine.reconstruct_host(pcms, param, residual=residual, want_pcm=want_pcm)
                    for i, c in enumerate(cases):
                        got = _as_tuple(stats[i])
                        where = (tile, residual, want_pcm, c["kind"], c["frames"], c["statistic"], c["tie"])
                        assert ob.stats_line(got) == c["stats_line"], where
                        if c["tie"]:
                            assert got == want[i], (where, [v.hex() for v in got], c["stats_hex"])
                        else:
                            assert got[2] == want[i][2], where
                            assert all(abs(g - w) <= float(reorder_bound(pcms[i].size)) * w for g, w in zip(got[:2], want[i][:2])), where
                        if want_pcm and not residual:
                            rec0 = out if rec0 is None else rec0
                            assert np.array_equal(out[i], rec0[i]), where
                        if want_pcm and residual:
                            assert np.array_equal(out[i], ob.residual(pcms[i], rec0[i])), where
        finally:
            engine.set_tile_kbytes(0)
    for i, c in enumerate(cases):
        assert np.array_equal(rec0[i], ob.decode(ob.encode(pcms[i], bits, block, 48000, ms, trials))[0]), c["frames"]
    # the same streams in a ragged, shuffled plan with short and segment-edge streams around them
    rng = np.random.default_rng(4100 + 10 * ch + bits)
    others = [synth_pcm(1, n, ch, seed=int(rng.integers(0, 1 << 30)), kind="music")[0] for n in (1, 5, 8192 // ch + 1, 40000, 991)]
    batch = pcms + others
    for residual in (False, True):
        rows, stats = _plan_run(engine, param, batch, residual, rng)
        for i, c in enumerate(cases):
            got = tuple(float(v) for v in stats[i])
            assert ob.stats_line(got) == c["stats_line"], (residual, c["frames"], c["statistic"])
            if c["tie"]:
                assert got == want[i], (residual, c["frames"], c["statistic"], [v.hex() for v in got], c["stats_hex"])
            want_row = ob.residual(pcms[i], rec0[i]) if residual else rec0[i]
            assert np.array_equal(rows[i], want_row), (residual, c["frames"])
        for j, x in enumerate(others):
            y = ob.decode(ob.encode(x, bits, block, 48000, ms, trials))[0]
            assert np.array_equal(rows[len(cases) + j], ob.residual(x, y) if residual else y), (residual, x.shape)
            assert ob.stats_line(tuple(float(v) for v in stats[len(cases) + j])) == ob.stats_line(ob.error_stats(x, y))


def _errors(x, y):
    """e per value, the reference's formula (src/main.c:470-491): every e is exact (correctly rounded division)"""
    gap = ((x.astype(np.int64) << 16) - (y.astype(np.int64) << 16)).astype(np.int32)
    return gap / 2147483647.0 - y.astype(np.float64) / 2147483647.0


@pytest.mark.parametrize("ch,bits", [(1, 4), (2, 3), (8, 2)])
def test_statistics_against_exact_sums(engine, ch, bits):
    """Default (tree) order against the EXACT statistics: e per value in numpy, the sums of e^2 and |e| exact (rational), the
    square root at 40 digits; |device - exact| <= delta(n) exact, with delta(n) the reordering bound proven in
    tests/test_compare_round.py, and MaxAE == max |e| (a maximum is order-free).  Ragged, shuffled batches at the compare kernels'
    geometry: value counts around one segment (kCompareSegment = 8192 values) and around 64 segments (the finish kernel's lane
    stride), one value, and one stream of about 3M values; decoded and residual output."""
    from decimal import Decimal, localcontext
    rng = np.random.default_rng(700 + ch)
    seg = 8192
    frames = [1, seg // ch - 1, seg // ch, seg // ch + 1, 64 * seg // ch - 1, 64 * seg // ch, 64 * seg // ch + 1, 3_000_000 // ch + 7]
    if ch == 1:
        assert frames[1:4] == [8191, 8192, 8193]
    pcms = [synth_pcm(1, n, ch, seed=int(rng.integers(0, 1 << 30)), kind=["noise", "music"][k % 2])[0] for k, n in enumerate(frames)]
    param = make_parameter(ch, bits, 1024, 48000, False, 0)
    ys = [ob.decode(ob.encode(x, bits, 1024))[0] for x in pcms]
    exact = []
    with localcontext() as ctx:
        ctx.prec = 40
        for x, y in zip(pcms, ys):
            e = _errors(x, y)
            n = x.size
            sq = sum(exact_sum(p) for p in exact_squares(e))
            ab = exact_sum(np.abs(e))
            rms = (Decimal(sq.numerator) / Decimal(sq.denominator) / n).sqrt()
            msd = Decimal(ab.numerator) / Decimal(ab.denominator) / n
            exact.append((rms, msd, float(np.max(np.abs(e))), Decimal(float(reorder_bound(n)))))
        for residual in (False, True):
            rows, stats = _plan_run(engine, param, pcms, residual, rng)
            for i, (x, y) in enumerate(zip(pcms, ys)):
                assert np.array_equal(rows[i], ob.residual(x, y) if residual else y), (ch, residual, frames[i])
                rms, msd, mx, d = exact[i]
                got = [float(v) for v in stats[i]]
                assert abs(Decimal(got[0]) - rms) <= d * rms, (ch, residual, frames[i], got[0], rms)
                assert abs(Decimal(got[1]) - msd) <= d * msd, (ch, residual, frames[i], got[1], msd)
                assert got[2] == mx, (ch, residual, frames[i], got[2], mx)


def test_reconstruct_argument_errors(engine):
    import ctypes as C
    lib, ctx = engine.lib, engine._ctx
    param = make_parameter(2, 4, 1024, 48000, False, 0)
    x = np.zeros((10, 2), dtype=np.int16)
    n = (C.c_uint32 * 1)(10)
    pp = (C.c_void_p * 1)(x.ctypes.data)
    assert lib.AADHip_ReconstructBatch(None, C.byref(param), 1, pp, n, 0, None, None) == 1
    assert lib.AADHip_ReconstructBatch(ctx, C.byref(param), 1, None, n, 0, None, None) == 1
    assert lib.AADHip_ReconstructBatch(ctx, C.byref(param), 1, pp, n, 7, pp, None) == 1          # unknown output kind
    bad = make_parameter(2, 5, 1024, 48000, False, 0)
    assert lib.AADHip_ReconstructBatch(ctx, C.byref(bad), 1, pp, n, 0, None, None) == 2          # INVALID_FORMAT
    assert lib.AADHip_ReconstructBatch(ctx, C.byref(param), 0, None, None, 0, None, None) == 0   # empty batch


def test_aad_batch_cli_reconstruction_modes(tmp_path):
    """aad_batch -r / -g / -c over ALL golden inputs in one invocation each (mono and stereo mixed),
    with two worker threads (-D 0,0: two contexts on the one GPU of the test box - the code path
    `-D 0,1,...` takes on a multi-GPU node) and the inputs given through a list file"""
    assert os.path.exists(CLI), "aad_batch not built"
    names, wavs = [], {}
    for c in CASES:
        if c["input"] not in wavs:
            _, _, data = cli_mode_input(c)
            path = tmp_path / (c["input"] + ".wav")
            path.write_bytes(data)
            wavs[c["input"]] = str(path)
            names.append(c["input"])
    listfile = tmp_path / "inputs.txt"
    listfile.write_text("\n".join(wavs[n] for n in names[1:]) + "\n")
    for bits, trials, ms in ((4, 2, False), (3, 0, True), (2, 2, False)):
        # the reference rejects M/S on mono input, and so does the engine: stereo inputs only there
        use = [n for n in names if not (ms and "mono" in n or ms and "_c1_" in n)]
        opts = ["-b", str(bits), "-t", str(trials), "-D", "0,0"] + (["-m"] if ms else [])
        want = {(c["input"]): c for c in CASES if (c["bits"], c["trials"], c["ms"]) == (bits, trials, ms)}
        rdir, gdir = tmp_path / ("r%d%d%d" % (bits, trials, ms)), tmp_path / ("g%d%d%d" % (bits, trials, ms))
        rdir.mkdir()
        gdir.mkdir()
        if use == names:
            files = ["-l", str(listfile), wavs[names[0]]]
        else:
            files = [wavs[n] for n in use]
        # the third parameter set with a forced tile size: the library's chunked staging and several device waves under the CLI
        env = dict(os.environ, AAD_HIP_TILE_KBYTES="3") if bits == 2 else None
        subprocess.run([CLI, "-r"] + opts + ["-o", str(rdir)] + files, check=True, env=env)
        subprocess.run([CLI, "--gap"] + opts + ["--output-dir", str(gdir)] + files, check=True, env=env)
        out = subprocess.run([CLI, "-c"] + opts + files, check=True, capture_output=True, text=True, env=env).stdout
        lines = dict(l.split("\t", 1) for l in out.splitlines(keepends=True))
        assert len(lines) == len(use)
        for n in use:
            assert sha256((rdir / (n + ".wav")).read_bytes()) == want[n]["reconstructed_sha256"], (n, bits)
            assert sha256((gdir / (n + ".wav")).read_bytes()) == want[n]["residual_sha256"], (n, bits)
            assert lines[wavs[n]] == want[n]["stats_line"], (n, bits)
