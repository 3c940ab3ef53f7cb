"""The wide resampler (AADHip_ResamplerCreateWide, include/aad_hip.h "resample"; aad_amd/csrc/aad_resample.h), what can be checked
without a device:
  * the symbol: the prototype in include/aad_hip.h and in HIP_SYMBOLS with AADHip_ResamplerCreate's seven arguments, a null
    handle refused;
  * the limits, through tests/resample_wide_driver.cpp (g++ over aad_resample.h): each refused once next to its largest accepted
    case - L 32768, 2 L K = 2 MiB, K = 256 - and zero ratios;
  * every ratio AADHip_ResamplerCreate accepts is accepted here too and flagged resident;
  * the library builder's banks for the ratios past the old limits against tests/resample_oracle.py: within 1 per coefficient,
    every phase sums to 16384, the mirror h[p][k] == h[L - p][K - 1 - k], sum |h| under the cap - all of the table
    but the 32768-phase bank, which takes numpy five seconds (its limits, plan and walk are checked);
  * the gather plan: R a multiple of 64 and at least 64, the rows and the phase index within kResampleGatherBytes and, with the
    span, within what a launch requests for such a resampler; and the walk of a tile as the gathered kernel makes it (the driver's
    `gather`), for every output of tiles 0 and 1: the output's row of its round holds the phase (n M) mod L;
  * the engine over the library that records its calls: wide=True reaches AADHip_ResamplerCreateWide with the ratios and select
    table the plain call hands to AADHip_ResamplerCreate, wide=False makes the call list of before, and mix_windows_resampled
    keeps its order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resample_oracle as ro
from aad_amd import capi
from test_engine_tensor_contract import CH, FRAMES, W, CpuEngine, FakeLib, header_bytes
from test_resample_host import RATIOS as PLAIN_RATIOS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "aad_hip.h")
# (up, down): K, bank bytes - the table of the issue; TABLE adds the 32768-phase bank, which no test here builds
WIDE = {(1600, 3969): (60, 192000), (1600, 4851): (74, 236800), (1600, 1617): (26, 83200), (1025, 1): (24, 49200),
        (1024, 1367): (34, 69632), (1025, 10933): (256, 524800), (3200, 8379): (64, 409600), (4099, 4098): (24, 196752)}
TABLE = dict(list(WIDE.items()) + [((32768, 32767), (24, 1572864))])
GATHER_BYTES = 40960
TILE = 1024


# ---- the symbol --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for name in ("AADHip_ResamplerCreate", "AADHip_ResamplerCreateWide"):
        m = re.search(r"AADApiResult\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m is not None, name
        protos[name] = re.sub(r"\s+", " ", m.group(1)).strip()
        assert name in capi.HIP_SYMBOLS
    assert len(protos["AADHip_ResamplerCreateWide"].split(",")) == 7
    assert protos["AADHip_ResamplerCreateWide"] == protos["AADHip_ResamplerCreate"]  # the arguments of AADHip_ResamplerCreate


def test_prototype_is_declared_on_the_library():
    lib = capi.load_library()
    fn = lib.AADHip_ResamplerCreateWide
    assert len(fn.argtypes) == 7 and list(fn.argtypes) == list(lib.AADHip_ResamplerCreate.argtypes) and fn.restype is C.c_int
    bad = capi.AADApiResult.INVALID_ARGUMENT
    assert fn(None, 0, None, 0, 1, None, None) == bad
    ratio = (capi.AADHipResampleRatio * 1)(capi.AADHipResampleRatio(1600, 3969))
    select = (C.c_uint16 * 1)(0)
    handle = C.c_void_p(0x55)
    assert fn(None, 1, ratio, 1, 1, select, C.byref(handle)) == bad and handle.value == 0x55  # no context: nothing written
    assert fn(C.c_void_p(1), 1, ratio, 1, 1, select, None) == bad  # no handle to return


# ---- the limits --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("resample_wide") / "resample_wide_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "resample_wide_driver.cpp")], check=True)
    return str(exe)


def _ask(driver, lines):
    out = subprocess.run([driver], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines)
    return out


def test_limits(driver):
    cases = [("0 5", "refused zero"), ("5 0", "refused zero"),
             ("32769 1", "refused 32769 1 24"), ("32768 32767", "ok 32768 32767 24 0 0"),     # L
             ("32768 43691", "refused 32768 43691 34"), ("32768 43689", "ok 32768 43689 32 0 0"),  # 2 L K: 2 MiB + 128 KiB, 2 MiB
             ("1025 11000", "refused 41 440 258"), ("1025 10933", "ok 1025 10933 256 0 0"),  # K
             ("1 11", "refused 1 11 264"), ("3 32", "ok 3 32 256 1 1"),                       # K, among the resident
             ("1025 1", "ok 1025 1 24 0 0"), ("1024 1", "ok 1024 1 24 1 1"),                  # one phase past the plain limit
             ("1024 1367", "ok 1024 1367 34 0 0"), ("1024 1365", "ok 1024 1365 32 1 1"),      # one tap pair past the plain bank
             ("160000 396900", "ok 1600 3969 60 0 0")]                                        # reduced before anything is counted
    out = _ask(driver, ["shape " + c[0] for c in cases])
    assert out == [c[1] for c in cases]
    assert 2 * 32768 * 32 == 2 << 20 and 2 * 32768 * 34 > 2 << 20


def test_table_of_the_issue(driver):
    table = TABLE
    out = _ask(driver, ["shape %d %d" % r for r in table])
    for (up, down), line in zip(table, out):
        K, size = table[(up, down)]
        assert line == "ok %d %d %d 0 0" % (up, down, K) and 2 * up * K == size and ro.taps(up, down) == K, (up, down, line)
        assert not ro.limits_ok(up, down)


def test_every_plain_ratio_is_accepted_and_resident(driver):
    rng = np.random.default_rng(3)
    ratios = list(PLAIN_RATIOS) + [(1024, 1023), (481, 1340), (1024, 1), (3, 32), (1024, 1365)]
    ratios += [(int(a), int(b)) for a, b in zip(rng.integers(1, 1100, size=400), rng.integers(1, 3000, size=400))]
    out = _ask(driver, ["shape %d %d" % r for r in ratios])
    plain = 0
    for (up, down), line in zip(ratios, out):
        if ro.limits_ok(up, down):
            plain += 1
            assert line.startswith("ok ") and line.endswith(" 1 1"), (up, down, line)
        elif line.startswith("ok "):
            assert line.endswith(" 0 0"), (up, down, line)  # wide alone: gathered
    assert plain > 60 and sum(line.endswith(" 0 0") for line in out) > 10 and sum(line.startswith("refused") for line in out) > 10


# ---- the banks ---------------------------------------------------------------------------------------------------------------------
def _check_bank(driver, up, down):
    v = np.array(_ask(driver, ["bank %d %d" % (up, down)])[0].split(), dtype=np.int64)
    L, M, K = (int(x) for x in v[:3])
    h = v[3:].reshape(L, K)
    assert (L, M) == (up, down) and K == ro.taps(L, M)
    assert (h.sum(axis=1) == 16384).all(), (up, down)
    assert (h[1:] == h[:0:-1, ::-1]).all(), (up, down)  # h[p][k] == h[L - p][K - 1 - k] for 0 < p < L
    most = int(np.abs(h).sum(axis=1).max())
    assert most <= 65535
    assert np.abs(h - ro.bank(L, M)).max() <= 1, (up, down)  # libm may move a largest-remainder choice
    return most


@pytest.mark.parametrize("ratio", list(WIDE), ids=["%d_%d" % r for r in WIDE])
def test_banks_against_the_oracles_construction(driver, ratio):
    most = _check_bank(driver, *ratio)
    assert 28000 <= most <= 33000  # a Kaiser-windowed sinc: about 2 * 16384 at the most, far from the cap


# ---- the gather plan ---------------------------------------------------------------------------------------------------------------
def _lds_stride(K):
    return K + 2 if (K // 2) % 2 == 0 else K


def _span_elements(L, M, K):
    return ((TILE - 1) * M // L + 1 + K + 1 + 2 + 1) // 2 * 2


def test_gather_plan(driver):
    table = dict(TABLE)
    table[(32768, 43689)] = (32, 2 << 20)
    out = _ask(driver, ["plan %d %d %d" % (L, M, K) for (L, M), (K, _) in table.items()])
    rounds = {}
    for ((L, M), (K, _)), line in zip(table.items(), out):
        R, rows, index, span = (int(v) for v in line.split())
        rounds[(L, M)] = R
        assert R % 64 == 0 and 64 <= R <= 256, (L, M, R)
        assert rows == 2 * R * _lds_stride(K) and index == 4 * R and span == 2 * _span_elements(L, M, K)
        assert (_lds_stride(K) // 2) % 2 == 1  # rows an odd number of words apart
        assert rows + index <= GATHER_BYTES, (L, M, K, R)
        assert R == 256 or 2 * R * (2 * _lds_stride(K) + 4) > GATHER_BYTES  # the largest round that fits
        # what a launch requests for a resampler of this bank alone: 2 * (bank_elements + span_elements) + 4 * round, below a CU's LDS
        request = 2 * (R * _lds_stride(K) + _span_elements(L, M, K)) + 4 * R
        assert rows + index + span <= request <= 160 * 1024 - 96
    assert rounds[(1600, 3969)] == 256 and rounds[(1600, 4851)] == 256 and rounds[(1025, 10933)] == 64 and rounds[(4099, 4098)] == 256
    # one resampler of all of them: the round of the bank with the most taps, the longest row, the longest span
    R = min(rounds.values())
    request = 2 * (R * max(_lds_stride(K) for K, _ in table.values()) + max(_span_elements(L, M, K) for (L, M), (K, _) in table.items())) + 4 * R
    assert request <= 64 * 1024


def test_gather_walk_publishes_each_outputs_phase(driver):
    table = dict(TABLE)
    table[(32768, 43689)] = (32, 2 << 20)
    asks = []
    for (L, M), (K, _) in table.items():
        for R in (64, 128, 256):  # a resampler's round is that of its bank with the most taps: any of the three for any bank
            for tile, T in ((0, 2048), (1, 2048), (0, 257), (1, 1025), (1, 1300), (0, 1), (0, 64), (0, 65)):
                asks.append((L, M, R, tile, T))
    out = _ask(driver, ["gather %d %d %d %d %d" % a for a in asks])
    for (L, M, R, tile, T), line in zip(asks, out):
        outputs = min(T - tile * TILE, TILE)
        assert line == "ok %d %d" % (outputs, -(-outputs // R)), (L, M, R, tile, T, line)


# ---- the engine, over the library that records its calls ------------------------------------------------------------------------------
T_SRC = 999
CREATES = ("AADHip_ResamplerCreate", "AADHip_ResamplerCreateWide")


class WideFakeLib(FakeLib):
    """FakeLib whose resamplers - of either constructor - hand out a handle, T_SRC source frames and a (1, 1) bank"""

    def __getattr__(self, name):
        call = FakeLib.__getattr__(self, name)

        def wrapped(*args):
            rc = call(*args)
            if name in CREATES:
                args[-1]._obj.value = 0x7000
            elif name == "AADHip_ResamplerSourceFrames":
                args[2]._obj.value = T_SRC
            elif name == "AADHip_ResamplerBank":
                args[2]._obj.value, args[3]._obj.value, args[4]._obj.value = 1, 1, 2
            return rc
        return wrapped


@pytest.fixture
def engine():
    e = CpuEngine.__new__(CpuEngine)
    e.torch, e.lib, e.device, e._ctx = torch, WideFakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def _corpus(rates):
    data = torch.zeros((len(rates), 64), dtype=torch.uint8)
    for row, rate in enumerate(rates):
        head = bytearray(header_bytes(CH, 100))
        head[18:22] = int(rate).to_bytes(4, "big")
        data[row, :31] = torch.frombuffer(head, dtype=torch.uint8)
    return data


def _trace(e, before):
    """the calls since `before`: names, and per create its (num_ratios, ratios, num_streams, variants, select entries)"""
    calls = e.lib.calls[before:]
    creates = []
    for name, a in calls:
        if name in CREATES:
            creates.append((a[1], [(r.up, r.down) for r in a[2]][:a[1]], a[3], a[4],
                            np.frombuffer(C.string_at(a[5], 2 * a[3] * a[4]), dtype=np.uint16).tolist()))
    return [c[0] for c in calls], creates


SPEEDS = ((9, 10), (1, 1), (11, 10))


def _entry_points(e):
    data, noise = _corpus((16000, 44100, 48000)), _corpus((44100, 16000))
    windows = torch.zeros((W, 2), dtype=torch.int64)
    spans = torch.zeros((W, 2), dtype=torch.int64)
    variant = torch.zeros(W, dtype=torch.int64)
    return {
        "resampler": lambda **k: e.resampler([(1600, 3969), (1, 1), (3, 2)], [[0, 1], [2, None]], **k).close(),
        "decode_windows_resampled": lambda **k: e.decode_windows_resampled(data, 64, windows, FRAMES, 16000, speeds=SPEEDS, variant=variant,
                                                                          dtype=torch.float16, **k),
        "window_levels_resampled": lambda **k: e.window_levels_resampled(data, 64, windows, FRAMES, 16000, speeds=SPEEDS, spans=spans, **k),
        "mix_windows_resampled": lambda **k: e.mix_windows_resampled((data, 64, windows), (noise, 64, windows), FRAMES, 6.0, 16000,
                                                                    speeds=SPEEDS, noise_spans=spans, dtype=torch.bfloat16, **k),
    }


@pytest.mark.parametrize("entry", ["resampler", "decode_windows_resampled", "window_levels_resampled", "mix_windows_resampled"])
def test_wide_reaches_the_wide_constructor_with_the_plain_calls_arguments(engine, entry):
    call = _entry_points(engine)[entry]
    traces = []
    for kwargs in ({}, dict(wide=False), dict(wide=True)):
        before = len(engine.lib.calls)
        call(**kwargs)
        traces.append(_trace(engine, before))
    (plain_names, plain_creates), (false_names, false_creates), (wide_names, wide_creates) = traces
    # wide=False is the call of before, name for name
    assert false_names == plain_names and false_creates == plain_creates
    assert "AADHip_ResamplerCreateWide" not in plain_names and plain_names.count("AADHip_ResamplerCreate") == len(plain_creates) >= 1
    # wide=True: the other constructor in the same places, the same ratios and select table, everything else alike
    assert wide_names == [n + "Wide" if n == "AADHip_ResamplerCreate" else n for n in plain_names]
    assert wide_creates == plain_creates
    if entry != "resampler":
        assert (1600, 3969) in plain_creates[0][1] and (1600, 4851) in plain_creates[0][1]


def test_wide_is_the_last_keyword():
    import inspect
    from aad_amd.engine import Engine
    for name in ("resampler", "decode_windows_resampled", "window_levels_resampled", "mix_windows_resampled", "_corpus_resampler"):
        p = list(inspect.signature(getattr(Engine, name)).parameters.values())[-1]
        assert p.name == "wide" and p.default is False, name


def test_mix_windows_resampled_keeps_its_order_when_wide(engine):
    before = len(engine.lib.calls)
    _entry_points(engine)["mix_windows_resampled"](wide=True)
    names, creates = _trace(engine, before)
    assert len(creates) == 2 and names.count("AADHip_ResamplerCreateWide") == 2 and "AADHip_ResamplerCreate" not in names
    work = [n for n in names if n in ("AADHip_ResamplerResolve", "AADHip_WindowDecodePlanRunStats", "AADHip_ResamplerRunStats",
                                      "AADHip_ResamplerRunGain", "AADHip_WindowDecodePlanRun", "AADHip_ResamplerRun")]
    # two resolves and two decodes with statistics (a pair per corpus), two statistics runs, then STORE and ADD
    assert work == ["AADHip_ResamplerResolve", "AADHip_WindowDecodePlanRunStats"] * 2 + ["AADHip_ResamplerRunStats"] * 2 + \
        ["AADHip_ResamplerRunGain"] * 2
    store, add = [c[1] for c in engine.lib.calls[before:] if c[0] == "AADHip_ResamplerRunGain"]
    assert store[11] == capi.WINDOW_GAIN_STORE and add[11] == capi.WINDOW_GAIN_ADD and store[9] == add[9]
    assert names[-4:] == ["AADHip_ResamplerDestroy", "AADHip_ResamplerDestroy", "AADHip_WindowDecodePlanDestroy", "AADHip_WindowDecodePlanDestroy"]
