"""The mix of the spectrogram stage (AADHip_SpectrogramRunMix, include/aad_hip.h "spectrogram", paragraph "mix"), what can be
checked without a device:
  * the symbol: the prototype in include/aad_hip.h and in HIP_SYMBOLS with its 12 arguments; a null handle refused;
  * aad_amd/csrc/aad_spectrogram.h's rule built with g++ into tests/spectrogram_mix_driver.cpp, against
    tests/spectrogram_mix_oracle.py: spectrum_mix_sample over rails, ties with even and odd floors, +-0, +-inf and NaN gains and
    random elements; spectrum_mix_span at its edges; spectrum_mix_rows, the argument check, against a brute force in Python
    integers;
  * the mutants: each of the nine mistakes a kernel could make changes an output bit of the inputs of a case of
    tests/test_gpu_spectrogram_mix.py - the fused multiply-add through planted witnesses, which random draws miss;
  * the witness census of those inputs: ties, clamps at each rail, elements inside and outside the span on both sides of the tile
    boundary, every count nonzero."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import spectrogram_matrix as sm
import spectrogram_mix_matrix as mm
import spectrogram_mix_oracle as mo
import spectrogram_oracle as so
from aad_amd import capi

HEADER = os.path.join(os.path.dirname(mm.HERE), "include", "aad_hip.h")
NAME = "AADHip_SpectrogramRunMix"


# ---- the symbol --------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"AADApiResult\s+%s\s*\(([^;]*)\)\s*;" % NAME, text)
    assert m is not None
    assert len(m.group(1).split(",")) == 12
    assert NAME in capi.HIP_SYMBOLS
    assert 'paragraph "mix"' in open(os.path.join(sm.CSRC, "aad_spectrogram.h")).read()


def test_the_prototype_is_declared_on_the_library():
    lib = capi.load_library()
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 12 and fn.restype is C.c_int
    assert fn(None, 1, None, 1, None, 1, 1, None, None, None, 1, None) == capi.AADApiResult.INVALID_ARGUMENT


# ---- the header's rule through g++ ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return mm.build_driver(tmp_path_factory.mktemp("spectrogram_mix"))


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    return str(tmp_path_factory.mktemp("spectrogram_mix_files"))


ELEMENT = np.dtype([("ga", np.float32), ("gb", np.float32), ("a", np.int16), ("b", np.int16), ("inside", np.int16), ("unused", np.int16)])


def _samples(driver, scratch, ga, a, gb, b, inside):
    rec = np.zeros(len(a), dtype=ELEMENT)
    rec["ga"], rec["gb"], rec["a"], rec["b"], rec["inside"] = ga, gb, a, b, inside
    src, dst = os.path.join(scratch, "elements.bin"), os.path.join(scratch, "samples.bin")
    rec.tofile(src)
    assert sm.ask(driver, "samples", len(rec), src, dst) == ["ok"]
    return np.fromfile(dst, dtype=np.int16)


def test_the_sample_rule_against_the_oracle(driver, scratch):
    inf, nan = np.inf, np.nan
    hand = [  # ga, a, gb, b, inside, the staged sample
        (1.0, 32767, 1.0, 32767, 1, 32767), (1.0, -32768, 1.0, -32768, 1, -32768), (1.0, 32767, 1.0, 1, 1, 32767),
        (1.0, 32767, 1.0, 32767, 0, 32767), (2.0, 20000, 1.0, 0, 0, 32767), (-2.0, 20000, 1.0, 0, 0, -32768),
        (0.5, 1, 0.5, 0, 1, 0), (0.5, 3, 0.5, 0, 1, 2), (0.5, 5, 0.5, 0, 1, 2), (0.5, -1, 0.5, 0, 1, 0), (0.5, -3, 0.5, 0, 1, -2),
        (0.5, 1, 0.5, 2, 1, 2), (0.5, 32767, 0.5, 32766, 1, 32766), (0.5, -32768, 0.5, -32767, 1, -32768),
        (0.5, 32767, 0.5, 0, 0, 16384), (0.5, 32765, 0.5, 0, 0, 16382),
        (0.0, 123, -0.0, 456, 1, 0), (-0.0, 123, 0.0, -456, 1, 0), (-0.0, -5, 1.0, 7, 0, 0),
        (inf, 1, 1.0, 5, 1, 32767), (-inf, 1, 1.0, 5, 1, -32768), (inf, -1, 1.0, 5, 0, -32768), (1.0, 5, inf, 3, 1, 32767),
        (1.0, 5, inf, 3, 0, 5), (inf, 0, 1.0, 5, 1, 0), (inf, 1, -inf, 1, 1, 0), (inf, 1, inf, 1, 1, 32767),
        (nan, 1, 1.0, 5, 1, 0), (nan, 1, 1.0, 5, 0, 0), (1.0, 5, nan, 3, 1, 0), (1.0, 5, nan, 3, 0, 5), (1.0, 5, nan, 0, 1, 0),
        (1e-45, 1, 1e-45, 1, 1, 0), (3.4e38, 32767, 3.4e38, 32767, 1, 32767), (3.4e38, 32767, -3.4e38, 32767, 1, 0),
    ]
    cols = list(zip(*hand))
    ga, a, gb, b, inside = (np.array(c) for c in cols[:5])
    want = np.array(cols[5], dtype=np.int16)
    with np.errstate(all="ignore"):
        assert np.array_equal(mo.mix_element(ga.astype(np.float32), a, gb.astype(np.float32), b, inside != 0), want)
        assert np.array_equal(_samples(driver, scratch, ga.astype(np.float32), a, gb.astype(np.float32), b, inside), want)
    # random elements under random and tie-making gains, and every b under the witnesses' gains
    rng = np.random.default_rng(7)
    n = 200000
    a, b = rng.integers(-32768, 32768, n).astype(np.int16), rng.integers(-32768, 32768, n).astype(np.int16)
    inside = rng.integers(0, 2, n)
    ga = np.where(rng.integers(0, 2, n) == 0, rng.choice([0.5, 0.25, 1.5, -0.5, 1.0], n), rng.normal(0, 1.2, n)).astype(np.float32)
    gb = np.where(rng.integers(0, 2, n) == 0, rng.choice([0.5, 0.25, 1.5, -0.5, 1.0], n), rng.normal(0, 1.2, n)).astype(np.float32)
    got = _samples(driver, scratch, ga, a, gb, b, inside)
    want = mo.mix_element(ga, a, gb, b, inside != 0)
    assert np.array_equal(got, want)
    assert (want == 32767).any() and (want == -32768).any()
    every = np.arange(-32768, 32768).astype(np.int16)
    for wa, wb in mm.fma_witnesses(*mm.WITNESS_GAINS, 4):
        av = np.full(every.shape, wa, dtype=np.int16)
        assert np.array_equal(_samples(driver, scratch, mm.WITNESS_GAINS[0], av, mm.WITNESS_GAINS[1], every, 1),
                              mo.mix_element(mm.WITNESS_GAINS[0], av, mm.WITNESS_GAINS[1], every, True))
        one = _samples(driver, scratch, mm.WITNESS_GAINS[0], [wa], mm.WITNESS_GAINS[1], [wb], 1)
        assert one[0] != mo.mix_element(mm.WITNESS_GAINS[0], [wa], mm.WITNESS_GAINS[1], [wb], True, "fma")[0]  # the header does not fuse


def test_the_span_rule_at_its_edges(driver):
    top = 2 ** 64 - 1
    for L, o, T in ((100, 0, 100), (100, 1, 100), (0, 5, 100), (top, 0, 100), (top, 99, 100), (top, 100, 100), (top, top, 100), (5, top, 100),
                    (2 ** 63, 2 ** 63, 100), (3, 97, 100), (4, 97, 100), (1, 99, 100), (7, 2 ** 32, 2 ** 32 - 1), (top, 1, 2 ** 32 - 1)):
        assert int(sm.ask(driver, "span", L, o, T)[0]) == mo.span_length(L, o, T), (L, o, T)
    assert mo.span_length(top, 99, 100) == 1 and mo.span_length(5, top, 100) == 0


def _rows_brute(num_rows, rows_a, pitch_a, rows_b, pitch_b, per, gain_a, gain_b, spans, T, out, W, H, columns, tile):
    """the refusals of section "mix" in Python integers -> "ok F tiles items" or "refused" """
    top = 2 ** 64
    if rows_a == 0 or rows_b == 0 or out == 0 or rows_a % 2 or rows_b % 2 or out % 4 or pitch_a < T or pitch_b < T or T < W:
        return "refused"
    F = 1 + (T - W) // H
    tiles = (F - 1) // tile + 1
    if num_rows * pitch_a * 2 >= top or num_rows * pitch_b * 2 >= top or num_rows * F * columns * 4 >= top or num_rows * tiles >= top:
        return "refused"
    if per == 0 or num_rows % per or gain_a % 4 or gain_b % 4 or spans % 8 or num_rows // per * 16 >= top:
        return "refused"
    return "ok %d %d %d" % (F, tiles, num_rows * tiles)


def test_the_argument_check_against_a_brute_force(driver):
    rows = lambda *a: sm.ask(driver, "rows", *a)[0]
    good = dict(num_rows=6, rows_a=0x1000, pitch_a=501, rows_b=0x2002, pitch_b=537, per=2, gain_a=0x3004, gain_b=0x4000, spans=0x5008,
                T=500, out=0x6004, W=400, H=160, columns=80, tile=256)
    assert rows(*good.values()) == _rows_brute(**good) == "ok 1 1 6"
    one_per_rule = [dict(rows_a=0), dict(rows_b=0), dict(out=0), dict(rows_a=0x1001), dict(rows_b=0x2001), dict(out=0x6002), dict(pitch_a=499),
                    dict(pitch_b=499), dict(T=399, pitch_a=399, pitch_b=399), dict(per=0), dict(per=4), dict(per=7), dict(gain_a=0x3002),
                    dict(gain_b=0x4001), dict(spans=0x5004), dict(num_rows=2 ** 63, per=1), dict(num_rows=2 ** 62, pitch_a=2, pitch_b=4, T=1, W=1, per=1)]
    for change in one_per_rule:
        args = dict(good, **change)
        assert rows(*args.values()) == _rows_brute(**args) == "refused", change
    for change in (dict(gain_a=0), dict(gain_b=0), dict(spans=0), dict(gain_a=0, gain_b=0, spans=0), dict(num_rows=0), dict(per=6), dict(per=1),
                   dict(rows_b=0x1000, pitch_b=501), dict(num_rows=0, per=5)):
        args = dict(good, **change)
        assert rows(*args.values()) == _rows_brute(**args) != "refused", change
    rng = np.random.default_rng(3)
    pick = lambda *values: int(values[rng.integers(len(values))])
    seen = set()
    for _ in range(150):
        T, W = pick(1, 400, 500, 2 ** 32 - 1), pick(1, 400, 401)
        args = dict(num_rows=pick(0, 1, 6, 12, 2 ** 31, 2 ** 40, 2 ** 61, 2 ** 62, 2 ** 63, 2 ** 64 - 1), rows_a=pick(0x1000, 0x1002, 0x1001, 0),
                    pitch_a=pick(T, T + 1, T - 1, 2 ** 33, 2 ** 63), rows_b=pick(0x2000, 0x2002, 0x2003, 0), pitch_b=pick(T, T + 37, 2 ** 62, 0),
                    per=pick(0, 1, 2, 3, 6, 2 ** 31, 2 ** 32 - 1), gain_a=pick(0, 0x3000, 0x3004, 0x3002), gain_b=pick(0, 0x4000, 0x4004, 0x4001),
                    spans=pick(0, 0x5000, 0x5008, 0x5004), T=T, out=pick(0x6000, 0x6004, 0x6002, 0), W=W, H=pick(1, 160, 2 ** 32 - 1),
                    columns=pick(1, 80, 2049), tile=pick(16, 256))
        want = _rows_brute(**args)
        assert rows(*args.values()) == want, args
        seen.add(want == "refused")
    assert seen == {True, False}


# ---- the mutants and the census, on the GPU cases' inputs ----------------------------------------------------------------------------
def _strided_inputs(a, b, parity):
    buf_a, at_a, pitch_a = sm.strided(a, mm.PITCH_EXTRA[0], parity[0])
    buf_b, at_b, pitch_b = sm.strided(b, mm.PITCH_EXTRA[1], parity[1])
    return buf_a, at_a, pitch_a, buf_b, at_b, pitch_b


@pytest.fixture(scope="module")
def gpu_inputs():
    """every run of test_small_every_edge and of the NaN and infinite gains case as mix_buffers' arguments:
    [(label, H or None, (buf_a, at_a, pitch_a, buf_b, at_b, pitch_b, R, T, rows_per_gain, gain_a, gain_b, spans))]"""
    runs = []
    for H in mm.SMALL_HOPS:
        T, a, b, cases = mm.small_cases(H)
        for label, gain_a, gain_b, spans in cases:
            runs.append(("H%d/%s" % (H, label), H, _strided_inputs(a, b, mm.PARITIES[0]) + (4, T, mm.ROWS_PER_GAIN, gain_a, gain_b, spans)))
    a, b, gain_a, gain_b = mm.special_gain_case()
    runs.append(("special", None, (a.reshape(-1), 0, a.shape[1], b.reshape(-1), 0, a.shape[1], a.shape[0], a.shape[1], 1, gain_a, gain_b, None)))
    return runs


@pytest.mark.parametrize("mutant", mo.MUTANTS)
def test_every_mutant_changes_an_output_bit_of_a_gpu_case(gpu_inputs, mutant):
    import test_gpu_spectrogram_mix as gpu
    assert callable(gpu.test_small_every_edge) and callable(gpu.test_nan_and_infinite_gains)
    window = so.hann(sm.SMALL_W)
    for label, H, args in gpu_inputs:
        x, y = mo.mix_buffers(*args), mo.mix_buffers(*args, mutant=mutant)
        if np.array_equal(x, y):
            continue
        H = 16 if H is None else H
        rows = np.flatnonzero((x != y).any(1))[:1]  # the spectrum of one changed row will do
        want, got = (so.spectrogram_rows(v[rows], window, sm.SMALL_FFT, H) for v in (x, y))
        if not np.array_equal(want.view(np.uint32), got.view(np.uint32)):
            print("%s: caught by %s, %d samples differ" % (mutant, label, int((x != y).sum())))
            return
    raise AssertionError("%s escapes every case: change the inputs, not the list" % mutant)


def test_the_planted_witnesses_are_the_fused_multiply_adds_only_ones():
    """without them the small case's random rows may well let the fused mutant pass: the planting is what the case relies on"""
    for H in mm.SMALL_HOPS:
        T, a, b = mm.small_rows(H)
        ga, gb = mm.WITNESS_GAINS
        differ = np.flatnonzero(mo.mix_element(ga, a[0], gb, b[0], True) != mo.mix_element(ga, a[0], gb, b[0], True, "fma"))
        assert set(mm.WITNESS_AT) <= set(differ.tolist())


def test_the_witness_census_of_the_small_case(driver):
    assert int(sm.ask(sm.build_driver(os.path.dirname(driver)), "constants")[0].split()[0]) == mm.SMALL_TILE_FRAMES
    for H in mm.SMALL_HOPS:
        T, a, b, cases = mm.small_cases(H)
        boundary = mm.SMALL_TILE_FRAMES * H
        total = {}
        for label, gain_a, gain_b, spans in cases:
            c = mo.census(a, b, mm.ROWS_PER_GAIN, gain_a, gain_b, spans, boundary)
            if label == "halves/whole":
                assert c["tie_even_floor"] and c["tie_odd_floor"], c
            if label == "signed/whole":
                assert c["clamp_low"] and c["clamp_high"], c
            if label.endswith("/edges"):  # the one span across the tile boundary, the other empty
                assert c["inside_before"] == 2 * mm.EDGE_BEFORE and c["inside_after"] == 2 * (mm.EDGE_L - mm.EDGE_BEFORE) and c["outside_before"] and c["outside_after"], c
            for k, v in c.items():
                total[k] = total.get(k, 0) + v
        print("H %d:" % H, total)
        assert all(v > 0 for v in total.values()), total
