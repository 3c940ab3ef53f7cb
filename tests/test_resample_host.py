"""The resample stage behind window decode (AADHip_Resampler*, include/aad_hip.h "resample"), what can be checked without a device:
  * the symbols: the six prototypes in include/aad_hip.h and in HIP_SYMBOLS, with their argument counts;
  * tests/resample_oracle.py pinned on hand-computed cases;
  * aad_amd/csrc/aad_resample.h - the reduction, the limits, the bank builder, the source batch's length and the resolve the
    kernel runs - built with g++ into tests/resample_policy_driver.cpp and held against the oracle's own construction and a brute
    force over the frames a window reads;
  * the quality of the library's banks, through the exact-integer oracle: tones in the passband and in the stopband;
  * the engine's routing and refusals, over the library that records its calls (tests/test_engine_tensor_contract.py).

The mirror property of a bank is h[p][k] == h[L - p][K - 1 - k] for 0 < p < L: tap k of phase p sits at
t = k - (K/2 - 1) - p / L and tap K - 1 - k of phase L - p at -t (K - 2 - k, at -t - 1, mirrors phase 0 onto itself).

Quality, as measured with the library's banks (dB, power ratios, the worst over the three frequencies; -s prints every figure):
  ratio      passband error   stopband level
  3/1           -84.7
  1/3           -83.1            -73.9
  160/147       -79.3
  147/160       -79.4            (its stopband tones lie above the source's Nyquist frequency: no such tone)
  10/9          -79.6
  10/11         -80.7            (as 147/160)
  160/441       -75.0            -76.3
The bound is -60 dB for both; coefficient rounding at Q14 is the floor."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resample_oracle as ro
from aad_amd import capi
from aad_amd.engine import run_extent
from test_engine_tensor_contract import CH, FRAMES, W, CpuEngine, FakeLib, _header, ragged_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "aad_hip.h")
RATIOS = [(1, 1), (3, 1), (1, 3), (160, 147), (147, 160), (10, 9), (10, 11), (160, 441)]
ARGUMENTS = {"AADHip_ResamplerCreate": 7, "AADHip_ResamplerDestroy": 1, "AADHip_ResamplerBank": 7, "AADHip_ResamplerSourceFrames": 3,
             "AADHip_ResamplerResolve": 7, "AADHip_ResamplerRun": 9}


# ---- the symbols -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, count in ARGUMENTS.items():
        m = re.search(r"(AADApiResult|void)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m is not None, name
        assert len(m.group(2).split(",")) == count, name
        assert name in capi.HIP_SYMBOLS
    run = re.search(r"AADHip_ResamplerRun\s*\(([^;]*)\)\s*;", text).group(1)
    assert run.index("device_source_rows") < run.index("source_frames") < run.index("device_lanes") < run.index("sample_type")
    assert C.sizeof(capi.AADHipResampleRatio) == 8 and [f[0] for f in capi.AADHipResampleRatio._fields_] == ["up", "down"]
    assert C.sizeof(capi.AADHipResampleLane) == 8 and [f[0] for f in capi.AADHipResampleLane._fields_] == ["bank", "shift"]
    assert capi.RESAMPLE_NO_BANK == 0xFFFF == ro.NO_BANK


def test_prototypes_are_declared_on_the_library():
    lib = capi.load_library()
    for name, count in ARGUMENTS.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == count, name
        assert fn.restype is (None if name.endswith("Destroy") else C.c_int), name
    assert lib.AADHip_ResamplerRun.argtypes[1] is C.c_uint64 and lib.AADHip_ResamplerRun.argtypes[7] is C.c_int32
    # no device is needed to be refused for a missing handle
    n = C.c_uint32(7)
    assert lib.AADHip_ResamplerSourceFrames(None, 10, C.byref(n)) == capi.AADApiResult.INVALID_ARGUMENT and n.value == 7
    assert lib.AADHip_ResamplerCreate(None, 0, None, 0, 1, None, None) == capi.AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_ResamplerRun(None, 1, 1, None, 1, None, 1, 0, None) == capi.AADApiResult.INVALID_ARGUMENT
    lib.AADHip_ResamplerDestroy(None)


# ---- the oracle, by hand -----------------------------------------------------------------------------------------------------------
def test_oracle_identity_returns_the_input():
    h = ro.bank(1, 1)
    assert h.tolist() == [[16384, 0]] and ro.taps(1, 1) == 2
    x = np.array([5, -7, 32767, -32768, 0, 1, -1], dtype=np.int16)
    for first in range(len(x) + 2):
        acc = ro.fir(x, first, 9, 1, 1, h)
        want = np.zeros(9, dtype=np.int64)
        part = x[first:first + 9]
        want[:len(part)] = part
        assert (acc == want * 16384).all()
        assert ro.convert(acc, "int16").tolist() == want.tolist()
        assert ro.convert(acc, "float32").tolist() == (want.astype(np.float32) / np.float32(32768)).view(np.uint32).tolist()
    assert not ro.fir(x, 2 ** 64 - 1, 4, 1, 1, h).any() and not ro.fir(x, -1, 4, 1, 1, h).any()  # huge and wrapped starts


def test_oracle_keeps_a_constant_where_the_taps_lie_inside_the_stream():
    x = np.full(400, 1000, dtype=np.int16)
    for L, M in ((3, 1), (1, 3)):
        h = ro.bank(L, M)
        K = h.shape[1]
        assert (h.sum(axis=1) == 16384).all()
        first, frames = 50, 60
        y = ro.convert(ro.fir(x, first, frames, L, M, h), "int16")
        n = np.arange(frames)
        lo = first + n * M // L - (K // 2 - 1)
        inside = (lo >= 0) & (lo + K <= len(x))
        assert inside.any() and (y[inside] == 1000).all()
        edge = ro.convert(ro.fir(x, 0, 8, L, M, h), "int16")  # the taps in front of frame 0 read zeros
        assert (edge != 1000).any()


def test_oracle_rounding_and_rails():
    c = lambda acc, t: ro.convert(np.array(acc, dtype=np.int64), t).tolist()
    # floor((acc + 8192) / 16384): halves go up, on both sides of zero
    assert c([8191, 8192, 24575, 24576, -8192, -8193, -24576, -24577, -1, 0], "int16") == [0, 1, 1, 2, 0, -1, -1, -2, 0, 0]
    # both rails: the largest accumulators, 32768 * 65535 on either side
    top = 32768 * 65535
    assert c([32767 * 16384 + 8191, 32767 * 16384 + 8192, top, -32768 * 16384 - 8192, -32768 * 16384 - 8193, -top], "int16") == \
        [32767, 32767, 32767, -32768, -32768, -32768]
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    assert c([16384, -16384, 1, 0, -1], "float32") == [f32(2.0 ** -15), f32(-2.0 ** -15), f32(2.0 ** -29), 0, f32(-2.0 ** -29)]
    assert c([(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1], "float32") == \
        [f32((1 << 24) * 2.0 ** -29), f32(((1 << 24) + 4) * 2.0 ** -29), f32(-(1 << 24) * 2.0 ** -29)]  # ties to even, then an exact scale
    assert c([16384 * 2049, 16384 * 2051, 0, -1], "float16") == [0x2C00, 0x2C02, 0, 0x8000]  # window decode's ties; -2^-29 -> -0
    assert c([16384 * 257, 16384 * 259, 0], "bfloat16") == [0x3C00, 0x3C02, 0]


def test_oracle_resolve_and_source_frames_by_hand():
    assert ro.resolve(0, 24) == (0, 0) and ro.resolve(1, 24) == (0, 1) and ro.resolve(10, 24) == (0, 10)
    assert ro.resolve(11, 24) == (0, 11) and ro.resolve(12, 24) == (1, 11) and ro.resolve(-1, 24) == (2 ** 64 - 12, 11)
    assert ro.resolve(5, 2) == (5, 0)
    assert ro.source_frames(257, [(1, 1, 2)]) == 258 and ro.source_frames(257, [(3, 1, 24)]) == 256 // 3 + 24
    assert ro.source_frames(257, [(1, 3, 72), (3, 1, 24)]) == 768 + 72
    assert ro.reduce_ratio(48000, 44100) == (160, 147) and ro.reduce_ratio(16000 * 10, 44100 * 11) == (1600, 4851)


# ---- aad_resample.h against numpy ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("resample") / "resample_policy_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "resample_policy_driver.cpp")], check=True)
    return str(exe)


def _ask(driver, lines):
    out = subprocess.run([driver], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def library_banks(driver):
    """(up, down) -> (L, M, int64 [L, K]): the banks the library builds, once"""
    banks = {}
    for r, line in zip(RATIOS, _ask(driver, ["bank %d %d" % r for r in RATIOS])):
        v = [int(t) for t in line.split()]
        banks[r] = (v[0], v[1], np.array(v[3:], dtype=np.int64).reshape(v[0], v[2]))
    return banks


def test_banks_against_the_oracles_construction(library_banks):
    for (up, down), (L, M, h) in library_banks.items():
        assert (L, M) == ro.reduce_ratio(up, down)
        K = h.shape[1]
        assert K == ro.taps(L, M) and K % 2 == 0
        if (L, M) != (1, 1):
            s = min(1.0, L / M)
            assert K == 2 * int(np.ceil(12 / s - 1e-9))
        assert (h.sum(axis=1) == 16384).all(), (up, down)
        assert np.abs(h).sum(axis=1).max() <= 65535
        for p in range(1, L):
            assert (h[p] == h[L - p][::-1]).all(), (up, down, p)  # h[p][k] == h[L - p][K - 1 - k]
        assert np.abs(h - ro.bank(L, M)).max() <= 1, (up, down)  # libm may move a largest-remainder choice
    assert library_banks[(1, 1)][2].tolist() == [[16384, 0]]


def test_limits(driver):
    cases = [("0 5", "refused zero"), ("5 0", "refused zero"),
             ("1025 1", "refused shape 1025 1 24"), ("1024 1", "ok 1024 1 24"),          # L
             ("1 11", "refused shape 1 11 264"), ("3 32", "ok 3 32 256"),                 # K
             ("1024 1367", "refused shape 1024 1367 34"), ("1024 1365", "ok 1024 1365 32"),  # 2 L K: 69632 and 65536 bytes
             ("96000 88200", "ok 160 147 24")]                                            # reduced before anything is counted
    out = _ask(driver, ["ratio " + c[0] for c in cases])
    for (ask, want), got in zip(cases, out):
        assert got.startswith(want), (ask, got)
        if want.startswith("ok"):
            # sum |h| <= 65535: a Kaiser-windowed sinc has an absolute sum of about 2 * 16384, so no ratio inside the other limits is
            # refused for it; the largest accepted cases are well below
            assert int(got.split()[-1]) <= 40000, (ask, got)
    for ask, _ in cases:
        up, down = (int(v) for v in ask.split())
        assert ro.limits_ok(up, down) == (not out[[c[0] for c in cases].index(ask)].startswith("refused"))


def test_source_frames_refusals(driver):
    out = _ask(driver, ["frames 0 1 1 2", "frames 1 3 4000000000 24", "frames 2 1 2147483647 24", "frames 2 1 2147483648 24",
                        "frames 2147483648 1 1 2", "frames 2147483649 1 1 2", "frames 2147483648 160 1 24"])
    assert out == ["refused", "24", str(2147483647 + 24), "refused", str(2147483647 + 2), "refused", str(2147483647 // 160 + 24)]


def test_resolve_and_source_frames_against_brute_force(driver, library_banks):
    banks = list(library_banks.values())
    lines = ["table 3 2 %d  0 1 2 3 4 65535  %s" % (len(banks), " ".join(str(h.shape[1] // 2 - 1) for _, _, h in banks))]
    select = [[0, 1], [2, 3], [4, 65535]]
    asks = []
    for stream in range(3):
        for variant in range(2):
            K = banks[select[stream][variant]][2].shape[1] if select[stream][variant] != 65535 else 2
            for first in list(range(K + 1)) + [10 ** 12, 2 ** 64 - 1]:
                asks.append((stream, first, variant))
    asks += [(3, 5, 0), (2 ** 64 - 1, 5, 0), (0, 5, 2), (0, 5, 2 ** 64 - 1), (2, 7, 1)]  # no stream, no variant, no bank
    lines += ["resolve %d %d %d" % a for a in asks]
    frames_asks = [(t, L, M, h.shape[1]) for L, M, h in banks for t in range(1, 41)]
    lines += ["frames %d %d %d %d" % a for a in frames_asks]
    out = _ask(driver, lines)
    assert out[0] == "ok"
    resolved = {}
    for (stream, first, variant), line in zip(asks, out[1:]):
        got = [int(v) for v in line.split()]
        if stream >= 3 or variant >= 2 or select[stream][variant] == 65535:
            assert got == [stream, first, 65535, 0]
            continue
        bank = select[stream][variant]
        K = banks[bank][2].shape[1]
        assert got == [stream, ro.resolve(first, K)[0], bank, ro.resolve(first, K)[1]]
        resolved[(bank, first)] = (got[1], got[3])
    t_src = {a: int(line) for a, line in zip(frames_asks, out[1 + len(asks):])}
    checked = 0
    for bank, (L, M, h) in enumerate(banks):
        K = h.shape[1]
        lead = K // 2 - 1
        for first in range(K + 1):
            if (bank, first) not in resolved:
                continue
            src_first, shift = resolved[(bank, first)]
            for t in range(1, 41):
                # every frame the definition reads: first + i + k - lead for n < t, k < K; in front of frame 0 it reads zeros
                read = [first + n * M // L + k - lead for n in range(t) for k in range(K)]
                assert src_first == max(min(read), 0)
                rows = t_src[(t, L, M, K)]
                assert rows == ro.source_frames(t, [(L, M, K)])
                assert max(read) - src_first <= rows - 1          # the source row holds the last frame read
                if first >= lead:
                    assert max(read) - src_first == rows - 1      # and not one more
                # the kernel's index: j = shift + i + k - lead is the frame's place in the source row, negative in front of frame 0
                assert all(shift + n * M // L + k - lead == f - src_first for f, (n, k) in
                           zip(read, ((n, k) for n in range(t) for k in range(K))))
                checked += 1
    assert checked > 1000


# ---- quality -----------------------------------------------------------------------------------------------------------------------
def _tone(freq, samples=8000, amplitude=20000):
    return np.round(amplitude * np.sin(2 * np.pi * freq * np.arange(samples))).astype(np.int16)


def _db(power_ratio):
    return 10 * np.log10(max(power_ratio, 1e-30))


def test_quality_of_the_library_banks(library_banks):
    """Tones of amplitude 20000, 8000 samples, through the library's banks in the integer oracle, int16 out; only outputs whose
    taps lie inside the stream count.  Passband, 0.05 / 0.2 / 0.35 cycles per sample of the lower rate: the error against the
    tone itself at the output's instants, its power over the tone's.  Stopband, 0.6 / 0.65 / 0.75 of the output rate, for the
    downsampling ratios and the tones the source rate can hold (below its Nyquist frequency): the output's power over the
    input's.  Both <= -60 dB."""
    worst_pass, worst_stop, stop_cases = -400.0, -400.0, 0
    for (up, down), (L, M, h) in library_banks.items():
        if (L, M) == (1, 1):
            continue
        K = h.shape[1]
        first = K
        frames = (8000 - 2 * K - first) * L // M
        t = first + np.arange(frames) * M / L  # the output's instants in source samples
        for f in (0.05, 0.2, 0.35):
            f_in = f if L >= M else f * L / M
            x = _tone(f_in)
            y = ro.convert(ro.fir(x, first, frames, L, M, h), "int16").astype(np.float64)
            ideal = 20000 * np.sin(2 * np.pi * f_in * t)
            level = _db(np.mean((y - ideal) ** 2) / np.mean(ideal ** 2))
            print("passband %d/%d f=%.2f: %.1f dB" % (up, down, f, level))
            worst_pass = max(worst_pass, level)
        if L < M:
            for f in (0.6, 0.65, 0.75):
                f_in = f * L / M
                if f_in >= 0.5:
                    continue  # no such tone at the source rate
                x = _tone(f_in)
                y = ro.convert(ro.fir(x, first, frames, L, M, h), "int16").astype(np.float64)
                level = _db(np.mean(y ** 2) / np.mean(x.astype(np.float64) ** 2))
                print("stopband %d/%d f=%.2f: %.1f dB" % (up, down, f, level))
                worst_stop = max(worst_stop, level)
                stop_cases += 1
    print("worst passband %.1f dB, worst stopband %.1f dB" % (worst_pass, worst_stop))
    assert stop_cases == 6  # 1/3 and 160/441
    assert worst_pass <= -60.0 and worst_stop <= -60.0


# ---- the engine, over the library that records its calls ------------------------------------------------------------------------------
T_SRC = 999


class ResampleFakeLib(FakeLib):
    """FakeLib whose resampler hands out a handle, T_SRC source frames and a (1, 1) bank"""

    def __getattr__(self, name):
        call = FakeLib.__getattr__(self, name)

        def wrapped(*args):
            rc = call(*args)
            if name == "AADHip_ResamplerCreate":
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
    e.torch, e.lib, e.device, e._ctx = torch, ResampleFakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def _setup(e):
    d = ragged_table()
    plan = e.window_decode_plan(_header(), d)
    res = e.resampler([(1, 1), (3, 2)], [[0, 1], [1, None], [0, 0]])
    good = dict(data=torch.zeros(run_extent("images", d), dtype=torch.uint8), windows=torch.zeros((W, 2), dtype=torch.int64),
                variant=torch.zeros(W, dtype=torch.int64), out=torch.zeros((W, CH, FRAMES), dtype=torch.float16))
    return plan, res, good


def test_resampler_create_hands_over_ratios_and_select(engine):
    _setup(engine)
    args = engine.lib.last("AADHip_ResamplerCreate")
    assert args[1] == 2 and [(r.up, r.down) for r in args[2]] == [(1, 1), (3, 2)] and args[3] == 3 and args[4] == 2
    assert np.frombuffer(C.string_at(args[5], 12), dtype=np.uint16).tolist() == [0, 1, 1, 0xFFFF, 0, 0]
    with pytest.raises(ValueError, match="select"):
        engine.resampler([(1, 1)], [[70000]])
    with pytest.raises(ValueError, match="ratios"):
        engine.resampler([(1 << 32, 1)], [[0]])


def test_run_is_resolve_window_decode_fir_in_that_order(engine):
    plan, res, good = _setup(engine)
    before = len(engine.lib.calls)
    out = res.run(plan, good["data"], good["windows"], FRAMES, variant=good["variant"], dtype=torch.float16, out=good["out"])
    assert out is good["out"]
    names = [c[0] for c in engine.lib.calls[before:]]
    assert names == ["AADHip_ResamplerSourceFrames", "AADHip_ResamplerResolve", "AADHip_WindowDecodePlanRun", "AADHip_ResamplerRun"]
    assert engine.lib.last("AADHip_ResamplerSourceFrames")[1] == FRAMES
    resolve = engine.lib.last("AADHip_ResamplerResolve")
    assert list(resolve[:5]) == [res.handle, W, good["windows"].data_ptr(), good["variant"].data_ptr(), FRAMES]
    decode = engine.lib.last("AADHip_WindowDecodePlanRun")
    # the source windows the resolve wrote, T_src frames, int16 rows
    assert list(decode[:6]) == [plan.handle, good["data"].data_ptr(), W, resolve[5], T_SRC, capi.SAMPLE_INT16]
    run = engine.lib.last("AADHip_ResamplerRun")
    assert list(run) == [res.handle, W, CH, decode[6], T_SRC, resolve[6], FRAMES, capi.SAMPLE_FLOAT16, good["out"].data_ptr()]
    # no variant table: NULL; no out: allocated, float32
    out = res.run(plan, good["data"], good["windows"], FRAMES)
    assert engine.lib.last("AADHip_ResamplerResolve")[3] is None
    assert out.dtype == torch.float32 and tuple(out.shape) == (W, CH, FRAMES)
    assert engine.lib.last("AADHip_ResamplerRun")[7:] == (capi.SAMPLE_FLOAT32, out.data_ptr())
    assert res.source_frames(5) == T_SRC and res.bank(0)[:2] == (1, 1)
    res.close()
    assert engine.lib.calls[-1][0] == "AADHip_ResamplerDestroy" and res.handle is None


REFUSALS = [
    ("windows", lambda g: g["windows"].to(torch.int32), "windows: dtype"),
    ("windows", lambda g: torch.zeros((W, 3), dtype=torch.int64), "windows: shape"),
    ("windows", lambda g: torch.zeros((W, 2), dtype=torch.int64, device="meta"), "windows: a tensor on the engine's device"),
    ("variant", lambda g: g["variant"].to(torch.int32), "variant: dtype"),
    ("variant", lambda g: torch.zeros(W + 1, dtype=torch.int64), "variant: shape"),
    ("variant", lambda g: torch.zeros(2 * W, dtype=torch.int64)[::2], "variant: a contiguous tensor"),
    ("variant", lambda g: torch.zeros(W, dtype=torch.int64, device="meta"), "variant: a tensor on the engine's device"),
    ("out", lambda g: g["out"].to(torch.float32), "out: dtype"),
    ("out", lambda g: torch.zeros((W, CH, FRAMES + 1), dtype=torch.float16), "out: shape"),
    ("out", lambda g: torch.zeros((W, CH, FRAMES + 3), dtype=torch.float16)[..., :FRAMES], "out: a contiguous tensor"),
    ("out", lambda g: torch.zeros((W, CH, FRAMES), dtype=torch.float16, device="meta"), "out: a tensor on the engine's device"),
]


@pytest.mark.parametrize("name,spoil,message", REFUSALS, ids=[r[2].replace(": ", "-").replace(" ", "_") for r in REFUSALS])
def test_run_refuses_a_tensor_off_its_contract(engine, name, spoil, message):
    plan, res, good = _setup(engine)
    before = len(engine.lib.calls)
    bad = dict(good, **{name: spoil(good)})
    with pytest.raises(ValueError, match=message):
        res.run(plan, bad["data"], bad["windows"], FRAMES, variant=bad["variant"], dtype=torch.float16, out=bad["out"])
    assert engine.lib.calls[before:] == []  # nothing reached the library
    with pytest.raises(ValueError, match="resample writes"):
        res.run(plan, good["data"], good["windows"], FRAMES, dtype=torch.float64)
    assert engine.lib.calls[before:] == []


def test_decode_windows_resampled_builds_ratios_from_the_headers(engine):
    from test_engine_tensor_contract import header_bytes
    data = torch.zeros((3, 64), dtype=torch.uint8)
    be = lambda v, n: int(v).to_bytes(n, "big")
    for row, rate in enumerate((16000, 44100, 48000)):
        head = bytearray(header_bytes(CH, 100))
        head[18:22] = be(rate, 4)
        data[row, :31] = torch.frombuffer(head, dtype=torch.uint8)
    windows = torch.zeros((W, 2), dtype=torch.int64)
    engine.decode_windows_resampled(data, 64, windows, FRAMES, 16000, speeds=((9, 10), (1, 1), (11, 10)))
    args = engine.lib.last("AADHip_ResamplerCreate")
    ratios = [(r.up, r.down) for r in args[2]][:args[1]]
    # rate * b / (sampling_rate * a), reduced: stream 0 at 16 kHz, stream 1 at 44.1 kHz, stream 2 at 48 kHz
    assert ratios == [(10, 9), (1, 1), (10, 11), (1600, 3969), (160, 441), (1600, 4851), (10, 27), (1, 3), (10, 33)]
    assert np.frombuffer(C.string_at(args[5], 18), dtype=np.uint16).tolist() == list(range(9))
    names = [c[0] for c in engine.lib.calls]
    assert names.index("AADHip_ResamplerResolve") < names.index("AADHip_WindowDecodePlanRun") < names.index("AADHip_ResamplerRun")
    assert names[-2:] == ["AADHip_ResamplerDestroy", "AADHip_WindowDecodePlanDestroy"]
    # equal reduced ratios share a bank
    engine.decode_windows_resampled(data[:1].expand(2, 64).contiguous(), 64, windows, FRAMES, 8000, speeds=((1, 1), (2, 2), (1, 2)))
    args = engine.lib.last("AADHip_ResamplerCreate")
    assert [(r.up, r.down) for r in args[2]][:args[1]] == [(1, 2), (1, 1)]
    assert np.frombuffer(C.string_at(args[5], 12), dtype=np.uint16).tolist() == [0, 0, 1, 0, 0, 1]
    with pytest.raises(ValueError, match="rate and speeds"):
        engine.decode_windows_resampled(data, 64, windows, FRAMES, 16000, speeds=((0, 1),))
