"""The spectrogram stage (AADHip_Spectrogram*, include/aad_hip.h "spectrogram"), what can be checked without a device:
  * the symbols: the five prototypes in include/aad_hip.h and in HIP_SYMBOLS with their argument counts; a null handle refused;
  * aad_amd/csrc/aad_spectrogram.h built with g++ into tests/spectrogram_driver.cpp, against tests/spectrogram_oracle.py: the
    quantised matrices everywhere for (n_fft 96, W 80), (512, 400) and (4096, 4096) with the periodic Hann window, q = 14; the
    byte planes against a brute-force matrix - pad rows and pad columns zero, Re and Im of a bin in the same column of two tiles;
    the column constants; the bands, packed weights and per-pair lists of the awkward filters (an all-zero one, an interior zero,
    a negative weight, one over every bin); F against a brute force over T in W .. W + 3 H; one refusal per rule with each
    limit's largest accepted case; the tile geometry;
  * the oracle's exact sums against Python integers on a rail row at W = 4096;
  * numpy mutants on the inputs of tests/test_gpu_spectrogram.py's cases: each of eight mistakes a kernel could make changes at
    least one output element of a named case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectrogram_matrix as sm
import spectrogram_oracle as so
from aad_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "aad_hip.h")
ARGUMENTS = {"AADHip_SpectrogramCreate": 8, "AADHip_SpectrogramDestroy": 1, "AADHip_SpectrogramFrames": 3,
             "AADHip_SpectrogramCoefficients": 4, "AADHip_SpectrogramRun": 6}
CONFIGS = ((96, 80), (512, 400), (4096, 4096))


# ---- the symbols -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, count in ARGUMENTS.items():
        m = re.search(r"(AADApiResult|void)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m is not None, name
        assert len(m.group(2).split(",")) == count, name
        assert name in capi.HIP_SYMBOLS


def test_prototypes_are_declared_on_the_library():
    lib = capi.load_library()
    for name, count in ARGUMENTS.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == count, name
        assert fn.restype is (None if name.endswith("Destroy") else C.c_int), name
    n = C.c_uint32(7)
    bad = capi.AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_SpectrogramFrames(None, 1000, C.byref(n)) == bad and n.value == 7
    assert lib.AADHip_SpectrogramCreate(None, 512, 400, 160, None, 0, None, None) == bad
    assert lib.AADHip_SpectrogramCoefficients(None, C.byref(n), None, 0) == bad and n.value == 7
    assert lib.AADHip_SpectrogramRun(None, 1, None, 1, 1, None) == bad
    lib.AADHip_SpectrogramDestroy(None)


# ---- aad_spectrogram.h through g++ ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return sm.build_driver(tmp_path_factory.mktemp("spectrogram"))


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    return str(tmp_path_factory.mktemp("spectrogram_files"))


def _coefficients(driver, scratch, window, n_fft):
    """-> (q, int16 [W, B, 2]) or the driver's refusal"""
    w, m = os.path.join(scratch, "window.bin"), os.path.join(scratch, "matrix.bin")
    np.asarray(window, dtype=np.float32).tofile(w)
    line = sm.ask(driver, "coefficients", n_fft, len(window), w, m)[0]
    if not line.startswith("ok"):
        return line
    assert line.split()[2:] == [], line
    return int(line.split()[1]), np.fromfile(m, dtype=np.int16).reshape(len(window), so.bins(n_fft), 2)


@pytest.fixture(scope="module")
def matrices(driver, scratch):
    return {cfg: _coefficients(driver, scratch, so.hann(cfg[1]), cfg[0]) for cfg in CONFIGS}


@pytest.mark.parametrize("cfg", CONFIGS, ids=["96x80", "512x400", "4096x4096"])
def test_the_quantised_matrices_equal_the_oracles_everywhere(matrices, cfg):
    n_fft, W = cfg
    q, m = matrices[cfg]
    oq, cq, sq = so.quantise(so.hann(W), n_fft)
    assert q == oq == 14
    assert np.array_equal(m[:, :, 0], cq) and np.array_equal(m[:, :, 1], sq)
    assert max(np.abs(cq).max(), np.abs(sq).max()) > 32639 // 2  # q + 1 would not fit


def test_the_quantiser_scale_ties_and_refusals(driver, scratch):
    # a flat window of 1.99 sits next to the bound at q = 14; 32639.4 fits q = 0 and 32639.6 does not
    for value, q in ((1.99, 14), (0.25, 15), (3.0, 13), (32639.4, 0)):
        got = _coefficients(driver, scratch, np.full(16, value, dtype=np.float32), 16)
        want = so.quantise(np.full(16, value, dtype=np.float32), 16)
        assert got[0] == want[0] == q and np.array_equal(got[1][:, :, 0], want[1]) and np.array_equal(got[1][:, :, 1], want[2])
    assert _coefficients(driver, scratch, np.full(16, 32639.6, dtype=np.float32), 16) == "refused"
    for spoil in (np.nan, np.inf, -np.inf):
        w = so.hann(16)
        w[5] = spoil
        assert _coefficients(driver, scratch, w, 16) == "refused"
    # ties to even: 2.5 * 2^-15 and 3.5 * 2^-15 at bin 0 (cos = 1) under q = 15
    got = _coefficients(driver, scratch, np.array([2.5 / 32768, 3.5 / 32768, 0.5], dtype=np.float32), 4)
    assert got[0] == 15 and got[1][:, 0, 0].tolist() == [2, 4, 16384]
    # the all-zero window: q = 15, every coefficient 0
    got = _coefficients(driver, scratch, np.zeros(8, dtype=np.float32), 8)
    assert got[0] == 15 and not got[1].any()


def test_shape_limits(driver):
    ok = lambda *a: sm.ask(driver, "shape", *a)[0] == "ok"
    assert ok(4096, 4096, 1) and ok(1, 1, 1) and ok(4096, 1, (1 << 32) - 1)
    assert not ok(4097, 4096, 1) and not ok(512, 513, 1) and not ok(512, 0, 1) and not ok(512, 400, 0)


def _planes(driver, scratch, m, n_fft):
    W = m.shape[0]
    src, dst = os.path.join(scratch, "cos_sin.bin"), os.path.join(scratch, "planes.bin")
    m.tofile(src)
    pairs, steps, nbytes = (int(v) for v in sm.ask(driver, "planes", n_fft, W, src, dst)[0].split())
    raw = np.fromfile(dst, dtype=np.uint8)
    assert raw.size == nbytes + 8 * 32 * pairs and nbytes == 2 * pairs * steps * 2048
    return pairs, steps, raw[:nbytes].view(np.int8), raw[nbytes:].view(np.int64).reshape(2, 16 * pairs)


@pytest.mark.parametrize("cfg", CONFIGS[:2], ids=["96x80", "512x400"])
def test_planes_and_constants_equal_a_brute_force_matrix(driver, scratch, matrices, cfg):
    n_fft, W = cfg
    q, m = matrices[cfg]
    B = so.bins(n_fft)
    pairs, steps, planes, consts = _planes(driver, scratch, m, n_fft)
    assert pairs == -(-B // 16) and steps == -(-W // 64)
    # the matrix the definition multiplies with: [64 steps, 2 pairs, 16], tile 2 c the cos and 2 c + 1 the -sin columns of
    # bins 16 c ..., rows t >= W and columns past B zero
    full = np.zeros((64 * steps, 2 * pairs, 16), dtype=np.int64)
    for k in range(B):
        full[:W, 2 * (k // 16), k % 16] = m[:, k, 0]
        full[:W, 2 * (k // 16) + 1, k % 16] = m[:, k, 1]
    p = planes.reshape(2 * pairs, steps, 2, 64, 16).astype(np.int64)  # tile, step, hh / hl, lane, element
    value = 256 * p[:, :, 0] + p[:, :, 1]
    lane, e = np.arange(64)[:, None], np.arange(16)[None, :]
    for ct in range(2 * pairs):
        for s in range(steps):
            want = full[64 * s + 16 * (lane >> 4) + e, ct, lane & 15]
            assert np.array_equal(value[ct, s], want), (ct, s)
    assert W % 64 != 0 and not value[:, steps - 1, 16 * ((W % 64 + 15) // 16):, :].any()  # pad rows
    if B % 16:
        assert not value[2 * pairs - 2:, :, :, :].reshape(2, steps, 4, 16, 16)[:, :, :, B % 16:, :].any()  # pad columns
    want = np.zeros((2, 16 * pairs), dtype=np.int64)
    want[:, :B] = 128 * m.astype(np.int64).sum(0).T
    assert np.array_equal(consts, want)


def test_bands_weights_and_lists_of_the_awkward_filters(driver, scratch):
    B, pairs = 49, 4
    f = sm.awkward_filters(B)
    src, dst = os.path.join(scratch, "filters.bin"), os.path.join(scratch, "weights.bin")
    f.tofile(src)
    lines = sm.ask(driver, "bands", 5, B, pairs, src, dst)
    got = [tuple(int(v) for v in line.split()) for line in lines[:5]]
    want = so.bands(f)
    assert want == [(49, 0), (3, 9), (13, 19), (0, 48), (47, 48)]
    assert [g[:2] for g in got] == want
    assert f[1, 6] == 0 and f[2, 15] < 0
    offsets, packed = [0, 0, 7, 14, 63], np.fromfile(dst, dtype=np.float32)
    assert [g[2] for g in got] == offsets and lines[5] == "total 65" and packed.size == 65
    for j, (lo, hi) in enumerate(want[1:], 1):
        assert np.array_equal(packed[offsets[j]:offsets[j] + hi - lo + 1].view(np.uint32), f[j, lo:hi + 1].view(np.uint32))
    lists = [[int(v) for v in line.split()[1:]] for line in lines[6:]]
    assert lists == [[j for j, (lo, hi) in enumerate(want) if (lo == B and c == 0) or (lo != B and lo <= 16 * c + 15 and hi >= 16 * c)]
                     for c in range(pairs)]
    assert lists == [[0, 1, 2, 3], [2, 3], [3, 4], [3, 4]]
    for spoil in (np.nan, np.inf, 2.0 ** -61, -2.0 ** -61):
        g = f.copy()
        g[2, 14] = spoil
        g.tofile(src)
        assert sm.ask(driver, "bands", 5, B, pairs, src, dst) == ["refused"]
    g = f.copy()
    g[2, 14] = 2.0 ** -60  # the least accepted weight
    g.tofile(src)
    assert sm.ask(driver, "bands", 5, B, pairs, src, dst)[5] == "total 65"


def test_frame_count_against_a_brute_force(driver):
    for W, H in ((80, 16), (80, 37), (400, 160), (16, 1), (4096, 512)):
        for T in range(W, W + 3 * H + 1, max(1, H // 7)):
            assert int(sm.ask(driver, "frames", T, W, H)[0]) == so.frame_counts(T, W, H) == so.frames(T, W, H), (T, W, H)
        assert sm.ask(driver, "frames", W - 1, W, H) == ["refused"]
    assert sm.ask(driver, "frames", (1 << 32) - 1, 1, 1) == [str((1 << 32) - 1)]


def test_one_refusal_per_rule_of_a_run(driver):
    rows = lambda *a: sm.ask(driver, "rows", *a)[0]
    # num_rows, rows, row_pitch, frames, out, W, H, columns, tile_frames
    assert rows(3, 0x1000, 500, 500, 0x2000, 400, 160, 80, 256) == "ok 1 1 3"
    assert rows(3, 0x1002, 400, 400, 0x2004, 400, 160, 80, 256) == "ok 1 1 3"  # 2-byte rows, 4-byte out, frames == W
    assert rows(2, 0x1000, 400 + 160 * 256, 400 + 160 * 256, 0x2000, 400, 160, 80, 256) == "ok 257 2 4"
    assert rows(0, 0x1000, 500, 500, 0x2000, 400, 160, 80, 256) == "ok 1 1 0"
    for refused in ((3, 0, 500, 500, 0x2000), (3, 0x1000, 500, 500, 0), (3, 0x1001, 500, 500, 0x2000), (3, 0x1000, 500, 500, 0x2002),
                    (3, 0x1000, 500, 399, 0x2000), (3, 0x1000, 499, 500, 0x2000)):
        assert rows(*refused, 400, 160, 80, 256) == "refused", refused
    # extents past 64 bits - the output's bytes, the rows' bytes - and the largest accepted of each
    assert rows(1 << 62, 0x1000, 1, 1, 0x2000, 1, 1, 1, 256) == "refused"
    assert rows((1 << 62) - 1, 0x1000, 1, 1, 0x2000, 1, 1, 1, 256).startswith("ok 1 1")
    assert rows(1 << 61, 0x1000, 1, 1, 0x2000, 1, 1, 2, 256) == "refused"
    assert rows((1 << 61) - 1, 0x1000, 1, 1, 0x2000, 1, 1, 2, 256).startswith("ok 1 1")
    assert rows(1 << 31, 0x1000, 1 << 32, 1, 0x2000, 1, 1, 1, 256) == "refused"
    assert rows(1 << 31, 0x1000, (1 << 32) - 1, 1, 0x2000, 1, 1, 1, 256).startswith("ok 1 1")


def test_tile_geometry(driver):
    tile, threads, span, max_fft = (int(v) for v in sm.ask(driver, "constants")[0].split())
    assert (tile, threads, max_fft) == (256, 256, 4096)
    for W, H in ((80, 16), (80, 37), (400, 160), (400, 441), (4096, 512), (4096, 4096), (16, 1), (64, 1 << 20), (4096, (1 << 32) - 1), (80, 65536)):
        pitch, frames, frame_major, elements, lds = sm.geometry(driver, W, H)
        steps = -(-W // 64)
        assert frames % 16 == 0 and 16 <= frames <= tile and pitch % 16 == 0
        assert elements == (frames - 1) * pitch + 64 * steps <= span           # the last fragment read ends inside the plane
        assert lds == 2 * elements + 4 * 17 * tile <= 160 * 1024
        assert pitch == (64 * steps if frame_major else H)
        if H % 16:
            assert frame_major
        if frames < tile:  # the largest that fits
            assert (frames + 16 - 1) * pitch + 64 * steps > span
    assert sm.geometry(driver, 400, 160)[:3] == (160, 256, 0) and sm.geometry(driver, 400, 441)[:3] == (448, 144, 1)


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------------
def test_the_oracles_sums_equal_python_integers_on_a_rail_row():
    row, window, q, cq, sq = sm.limit_inputs()
    Re, Im = so.sums(row[0], cq, sq, sm.LIMIT_H)
    x = [int(v) for v in row[0]]
    for f, k in ((0, 5), (1, 5), (0, 0), (1, 2048), (0, 1000)):
        assert int(Re[f, k]) == sum(x[f * sm.LIMIT_H + t] * int(cq[t, k]) for t in range(4096)), (f, k)
        assert int(Im[f, k]) == sum(x[f * sm.LIMIT_H + t] * int(sq[t, k]) for t in range(4096)), (f, k)
    assert 0.6 * 2 ** 42 < abs(int(Re[0, 5])) < 2 ** 42
    assert so.element(np.array([(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1]), 14).tolist() == [2.0 ** -5, (2.0 ** 24 + 4) * 2.0 ** -29, -2.0 ** -5]


def test_frame_counts_and_mel_filters_of_the_oracle():
    assert [so.frame_counts(c, 400, 160) for c in (0, 399, 400, 559, 560, 4000)] == [0, 0, 1, 1, 2, 23]
    f = so.mel_filters(16000, 512, 80)
    assert f.shape == (80, 257) and f.dtype == np.float32 and (f >= 0).all() and f.max() <= 1
    lo_hi = so.bands(f)
    assert all(lo <= hi for lo, hi in lo_hi) and [lo for lo, _ in lo_hi] == sorted(lo for lo, _ in lo_hi)
    assert not f[:, 0].any()  # f_min = 0: the first triangle's foot


# ---- mutants: what the GPU cases must catch ------------------------------------------------------------------------------------------
# mutant -> the case of tests/test_gpu_spectrogram.py (hop, with filters) whose output it changes
MUTANT_CASES = {"no_constant": (16, False), "stride_w": (16, False), "late": (37, False), "fma": (80, False), "exact_square": (96, False),
                "descending": (16, True), "neighbour_tile": (37, False), "first_span": (80, True)}


@pytest.fixture(scope="module")
def small_cases(driver):
    out = {}
    for H, with_filters in set(MUTANT_CASES.values()):
        tile = sm.geometry(driver, sm.SMALL_W, H)[1]
        rows = sm.hand_made_rows(sm.small_frames(H, tile))
        filters = sm.awkward_filters(so.bins(sm.SMALL_FFT)) if with_filters else None
        out[(H, with_filters)] = (rows, filters, tile, so.spectrogram_rows(rows, so.hann(sm.SMALL_W), sm.SMALL_FFT, H, filters))
    return out


@pytest.mark.parametrize("mutant", so.MUTANTS)
def test_every_mutant_changes_an_output_of_a_named_case(small_cases, mutant):
    import test_gpu_spectrogram as gpu
    assert callable(gpu.test_small_every_edge) and set(MUTANT_CASES) == set(so.MUTANTS)
    H, with_filters = MUTANT_CASES[mutant]
    assert H in sm.SMALL_HOPS
    rows, filters, tile, want = small_cases[(H, with_filters)]
    got = so.spectrogram_rows(rows, so.hann(sm.SMALL_W), sm.SMALL_FFT, H, filters, mutant, tile)
    assert got.shape == want.shape
    changed = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(mutant, "changes", changed, "of", want.size, "elements")
    assert changed > 0
