"""The convolve stage behind window decode (AADHip_Convolver*, include/aad_hip.h "reverberation"), what can be checked without a
device:
  * the symbols: the seven prototypes in include/aad_hip.h and in HIP_SYMBOLS, with their argument counts; a null handle refused;
  * aad_amd/csrc/aad_convolve.h built with g++ into tests/convolve_driver.cpp: the quantiser against tests/convolve_oracle.py - q
    for the peaks 1.0, 0.996, 0.25, 3.0 and 32639.4, the refusals at 32639.6, NaN and inf, ties to even at x.5 * 2^-q, the all-zero
    response, the default delay's tie rule; the byte split of every tap in the bound and of every sample; the planes of B against
    a brute-force Hankel matrix for K = 1, 17, 64, 65 and 1000 with the constant 128 sum h; the resolve and T_src against a brute
    force over every frame a window reads; the elements;
  * the oracle pinned on hand-computed cases: the identity, both rails, the int16 rounding of negative sums at Q = 0 and Q = 15,
    the float32 ties 2^24 + 1 and 2^24 + 3;
  * the engine's call order and refusals over the library that records its calls (tests/test_engine_tensor_contract.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import convolve_oracle as co
from aad_amd import capi
from aad_amd.engine import ConvolveSource, run_extent
from test_engine_tensor_contract import CH, FRAMES, W, CpuEngine, FakeLib, _header, ragged_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "aad_hip.h")
ARGUMENTS = {"AADHip_ConvolverCreate": 6, "AADHip_ConvolverDestroy": 1, "AADHip_ConvolverResponse": 7, "AADHip_ConvolverSourceFrames": 3,
             "AADHip_ConvolverResolve": 7, "AADHip_ConvolverRun": 9, "AADHip_ConvolverRunGain": 12}


# ---- the symbols -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, count in ARGUMENTS.items():
        m = re.search(r"(AADApiResult|void)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m is not None, name
        assert len(m.group(2).split(",")) == count, name
        assert name in capi.HIP_SYMBOLS
    gain = re.search(r"AADHip_ConvolverRunGain\s*\(([^;]*)\)\s*;", text).group(1)
    assert gain.index("device_lanes") < gain.index("device_spans") < gain.index("sample_type") < gain.index("device_gain") < gain.index("mode")
    assert C.sizeof(capi.AADHipConvolveLane) == 8 and [f[0] for f in capi.AADHipConvolveLane._fields_] == ["response", "shift"]


def test_prototypes_are_declared_on_the_library():
    lib = capi.load_library()
    for name, count in ARGUMENTS.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == count, name
        assert fn.restype is (None if name.endswith("Destroy") else C.c_int), name
    n = C.c_uint32(7)
    bad = capi.AADApiResult.INVALID_ARGUMENT
    assert lib.AADHip_ConvolverSourceFrames(None, 10, C.byref(n)) == bad and n.value == 7
    assert lib.AADHip_ConvolverCreate(None, 0, None, None, None, None) == bad
    assert lib.AADHip_ConvolverResponse(None, 0, C.byref(n), C.byref(n), C.byref(n), None, 0) == bad and n.value == 7
    assert lib.AADHip_ConvolverResolve(None, 1, None, None, 1, None, None) == bad
    assert lib.AADHip_ConvolverRun(None, 1, 1, None, 1, None, 1, 0, None) == bad
    assert lib.AADHip_ConvolverRunGain(None, 1, 1, None, 1, None, None, 1, 1, None, None, 0) == bad
    lib.AADHip_ConvolverDestroy(None)


# ---- aad_convolve.h through g++ -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("convolve") / "convolve_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "convolve_driver.cpp")],
                   check=True)
    return str(exe)


def _ask(driver, lines):
    out = subprocess.run([driver], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout
    out = out.splitlines()
    assert len(out) == len(lines)
    return out


def _quantise(driver, h, delay=-1):
    h = np.asarray(h, dtype=np.float32)
    line = _ask(driver, ["q %d %d %s" % (delay, h.size, " ".join("%08x" % b for b in h.view(np.uint32)))])[0]
    if line == "refused":
        return None
    words = line.split()
    assert words[0] == "ok" and len(words) == 3 + h.size, line
    return np.array(words[3:], dtype=np.int64), int(words[1]), int(words[2])


def _same(got, want):
    if want is None:
        return got is None
    return got is not None and got[0].tolist() == want[0].astype(np.int64).tolist() and got[1:] == want[1:]


def test_quantiser_scale_per_peak(driver):
    for peak, q in ((1.0, 14), (0.996, 15), (0.25, 15), (3.0, 13), (32639.4, 0)):
        h = np.array([0.0, peak / 3, -peak, peak / 7], dtype=np.float32)
        got, want = _quantise(driver, h), co.quantise(h)
        assert want[1] == q and want[2] == 2 and _same(got, want), (peak, got, want)
    # the identity: the bound, not 2^15, sets the scale
    assert _quantise(driver, [1.0])[0].tolist() == [16384] and _quantise(driver, [1.0])[1:] == (14, 0)
    assert _quantise(driver, [-1.0])[0].tolist() == [-16384]
    # 32639 is the largest tap: 32639 * 2^-15 keeps q = 15, one more step of 2^-15 loses a bit
    assert _quantise(driver, [32639 / 32768])[1] == 15 and _quantise(driver, [32640 / 32768])[1] == 14


def test_quantiser_refusals(driver):
    assert co.quantise([32639.6]) is None and _quantise(driver, [32639.6]) is None
    assert _quantise(driver, [0.5, -32640.0]) is None and co.quantise([0.5, -32640.0]) is None
    for bad in (np.nan, np.inf, -np.inf):
        assert _quantise(driver, [0.25, bad, 0.5]) is None and co.quantise([0.25, bad, 0.5]) is None
    assert _ask(driver, ["q -1 0", "q -1 32769"]) == ["refused", "refused"]
    assert co.quantise(np.zeros(0)) is None and co.quantise(np.zeros(32769)) is None
    assert _quantise(driver, [1.0, 0.5], delay=2) is None and co.quantise([1.0, 0.5], delay=2) is None
    top = np.zeros(32768, dtype=np.float32)
    top[-1] = 0.5
    assert _same(_quantise(driver, top), co.quantise(top)) and co.quantise(top)[2] == 32767


def test_quantiser_ties_to_even_and_zero(driver):
    # with the peak 0.75 (q = 15), x.5 * 2^-15 lies exactly between two taps: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0, -1.5 -> -2
    h = np.array([0.75, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, -2.5 / 32768, 3.5 / 32768], dtype=np.float32)
    got = _quantise(driver, h)
    assert got[1] == 15 and got[0].tolist() == [24576, 0, 2, 2, 0, -2, -2, 4] and _same(got, co.quantise(h))
    zero = _quantise(driver, np.zeros(5))
    assert zero[0].tolist() == [0] * 5 and zero[1:] == (15, 0) and _same(zero, co.quantise(np.zeros(5)))


def test_default_delay_is_the_first_largest_tap(driver):
    h = np.array([0.1, -0.5, 0.5, 0.5, 0.2], dtype=np.float32)
    assert _quantise(driver, h)[2] == 1 == co.quantise(h)[2]
    assert _quantise(driver, h, delay=4)[2] == 4 == co.quantise(h, 4)[2]
    assert _quantise(driver, h, delay=0)[2] == 0 == co.quantise(h, 0)[2]
    # a tie that only the quantised taps show: 0.50001 and 0.5 round to the same tap at q = 15
    near = np.array([0.0, 0.5, 0.5 + 2.0 ** -20], dtype=np.float32)
    assert _quantise(driver, near)[2] == 1 == co.quantise(near)[2]


def test_every_tap_and_sample_splits_into_two_signed_bytes(driver):
    assert _ask(driver, ["split"]) == ["ok"]


@pytest.mark.parametrize("K", [1, 17, 64, 65, 1000])
def test_planes_equal_a_brute_force_hankel_matrix(driver, K):
    rng = np.random.default_rng(K)
    taps = rng.integers(-co.MAX_TAP, co.MAX_TAP + 1, size=K)
    taps[0], taps[-1] = co.MAX_TAP, -128  # hh = hl = 127; hl = -128
    steps, bias, raw = _ask(driver, ["planes %d %s" % (K, " ".join(str(int(t)) for t in taps))])[0].split()
    steps = int(steps)
    assert steps == (K + 15 + 63) // 64 and int(bias) == 128 * int(taps.sum())
    got = np.frombuffer(bytes.fromhex(raw), dtype=np.int8)
    assert (got[steps * 2048:] == 0x5A).all() and len(got) == steps * 2048 + 16
    got = got[:steps * 2048].reshape(steps, 2, 64, 16).astype(np.int64)
    # B_s[u][j] = h[K - 1 - (64 s + u - j)], 0 outside the response; lane l holds B_s[16 (l >> 4) + e][l & 15] at byte e
    for s in range(steps):
        for lane in range(64):
            for e in range(16):
                t = 64 * s + 16 * (lane >> 4) + e - (lane & 15)
                h = int(taps[K - 1 - t]) if 0 <= t < K else 0
                assert 256 * got[s, 0, lane, e] + got[s, 1, lane, e] == h, (s, lane, e)
    # every tap stands in every column exactly once
    assert (256 * got[:, 0] + got[:, 1]).sum() == 16 * taps.sum()


def test_resolve_and_source_frames_against_every_frame_a_window_reads(driver):
    responses = [(np.ones(1), 14, 0), (np.ones(24), 0, 0), (np.ones(24), 0, 23), (np.ones(24), 0, 7), (np.ones(100), 0, 40)]
    lead = [len(t) - 1 - d for t, _, d in responses]
    frames = 37
    t_src = co.source_frames(frames, responses)
    assert _ask(driver, ["source %d 100" % frames, "source 0 100", "source 1 1", "source 4294967295 32768"]) == \
        [str(t_src), "refused", "1", str(4294967295 + 32767)]
    firsts = [0, 1, 15, 16, 17, 22, 23, 24, 58, 59, 60, 61, 5000, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 30]
    lines, cases = [], []
    for r in list(range(len(responses))) + [len(responses), (1 << 64) - 1, 1 << 40]:
        for first in firsts:
            lines.append("resolve 3 %d %d %d %s" % (first, r, len(responses), " ".join(map(str, lead))))
            cases.append((first, r))
    for (first, r), line in zip(cases, _ask(driver, lines)):
        stream, src_first, lane, shift = [int(v) for v in line.split()]
        assert (stream, src_first, lane, shift) == co.resolve(3, first, r, responses), (first, r)
        if lane == co.NO_RESPONSE:
            assert (src_first, shift) == (first, 0)
            continue
        taps, _, d = responses[r]
        K = len(taps)
        # brute force: every frame the window reads is a frame of the source row, or lies in front of frame 0
        for n in (0, 1, frames - 1):
            for k in range(K):
                frame = first + n + d - k  # of the stream, when the window does not wrap
                j = shift + n + d - k
                assert j < t_src
                if first < (1 << 62):
                    assert (j < 0) == (frame < 0) and (j < 0 or src_first + j == frame)
        assert shift == min(first, lead[r]) and src_first == first - shift


def test_elements_equal_the_oracle(driver):
    accs = [0, 1, -1, (1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 44) + 12345, -(1 << 44) - 99999, 32767 << 15, -(32768 << 15) - 1]
    lines = ["element %d %d" % (a, q) for a in accs for q in (0, 1, 14, 15)]
    for line, (a, q) in zip(_ask(driver, lines), [(a, q) for a in accs for q in (0, 1, 14, 15)]):
        i16, f32 = line.split()
        assert int(i16) == int(co.to_int16([a], q)[0]) and int(f32, 16) == int(co.to_float32([a], q).view(np.uint32)[0]), (a, q)


# ---- the oracle, by hand -----------------------------------------------------------------------------------------------------------
def test_oracle_identity_returns_the_input():
    taps, q, d = co.quantise([1.0])
    assert taps.tolist() == [16384] and (q, d) == (14, 0)
    x = np.array([5, -7, 32767, -32768, 0, 1, -1], dtype=np.int16)
    for first in range(len(x) + 2):
        acc = co.row(x, len(x), first, 9, (taps, q, d))
        want = np.zeros(9, dtype=np.int64)
        part = x[first:first + 9]
        want[:len(part)] = part
        assert (acc == want * 16384).all()
        assert co.to_int16(acc, q).tolist() == want.tolist()
        assert co.to_float32(acc, q).tolist() == (want.astype(np.float32) / np.float32(32768)).tolist()
    assert not co.row(x, len(x), (1 << 64) - 1, 4, (taps, q, d)).any() and not co.row(x, len(x), -1, 4, (taps, q, d)).any()
    assert not co.row(x, len(x), 0, 4, None).any()


def test_oracle_delay_moves_the_direct_path():
    x = np.arange(1, 11, dtype=np.int16)
    taps = np.array([0, 0, 3, 0, 1], dtype=np.int64)
    # delay 2: output n = 3 x[n] + x[n - 2]
    acc = co.sums(x, 0, 10, taps, 2)
    assert acc.tolist() == [3 * x[n] + (x[n - 2] if n >= 2 else 0) for n in range(10)]
    # delay 0: output n = 3 x[n - 2] + x[n - 4]; delay K - 1: output n = 3 x[n + 2] + x[n]
    assert co.sums(x, 4, 3, taps, 0).tolist() == [3 * x[2] + x[0], 3 * x[3] + x[1], 3 * x[4] + x[2]]
    assert co.sums(x, 7, 3, taps, 4).tolist() == [3 * x[9] + x[7], x[8], x[9]]


def test_oracle_rounding_and_rails():
    c = lambda acc, q: co.to_int16(np.array(acc, dtype=np.int64), q).tolist()
    assert c([-1, 0, 1, -32768, 32767, -32769, 32768], 0) == [-1, 0, 1, -32768, 32767, -32768, 32767]  # Q = 0: no rounding term
    h = 1 << 14
    assert c([h - 1, h, 3 * h - 1, 3 * h, -h, -h - 1, -3 * h, -3 * h - 1, -1, 0], 15) == [0, 1, 1, 2, 0, -1, -1, -2, 0, 0]
    top = 32768 * 32639 * 32768
    assert top < 1 << 45
    assert c([(32767 << 15) + h - 1, (32767 << 15) + h, top, -(32768 << 15) - h, -(32768 << 15) - h - 1, -top], 15) == \
        [32767, 32767, 32767, -32768, -32768, -32768]
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    bits = lambda acc, q: co.element_bits(np.array(acc, dtype=np.int64), q, "float32").tolist()
    assert bits([16384, -16384, 1, 0, -1], 14) == [f32(2.0 ** -15), f32(-2.0 ** -15), f32(2.0 ** -29), 0, f32(-2.0 ** -29)]
    for q in (0, 15):
        assert bits([(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 44) + (1 << 20), (1 << 44) + 3 * (1 << 20)], q) == \
            [f32((1 << 24) * 2.0 ** -(15 + q)), f32(((1 << 24) + 4) * 2.0 ** -(15 + q)), f32(-(1 << 24) * 2.0 ** -(15 + q)),
             f32((1 << 44) * 2.0 ** -(15 + q)), f32(((1 << 44) + (1 << 22)) * 2.0 ** -(15 + q))]  # ties to even, then an exact scale
    assert co.element_bits(np.array([16384 * 2049, 16384 * 2051, 0, -1]), 14, "float16").tolist() == [0x2C00, 0x2C02, 0, 0x8000]
    assert co.element_bits(np.array([16384 * 257, 16384 * 259, 0]), 14, "bfloat16").tolist() == [0x3C00, 0x3C02, 0]


# ---- the engine, over the library that records its calls ------------------------------------------------------------------------------
T_SRC = 999


class ConvolveFakeLib(FakeLib):
    """FakeLib whose convolver hands out a handle and T_SRC source frames"""

    def __getattr__(self, name):
        call = FakeLib.__getattr__(self, name)

        def wrapped(*args):
            rc = call(*args)
            if name == "AADHip_ConvolverCreate":
                args[-1]._obj.value = 0x7100
            elif name == "AADHip_ConvolverSourceFrames":
                args[2]._obj.value = T_SRC
            return rc
        return wrapped


@pytest.fixture
def engine():
    e = CpuEngine.__new__(CpuEngine)
    e.torch, e.lib, e.device, e._ctx = torch, ConvolveFakeLib(), 0, C.c_void_p(1)
    e.tensor_device = torch.device("cpu")
    return e


def _setup(e):
    d = ragged_table()
    plan = e.window_decode_plan(_header(), d)
    conv = e.convolver([[1.0], [0.5, 0.25, -0.125]], delays=[None, 2])
    good = dict(data=torch.zeros(run_extent("images", d), dtype=torch.uint8), windows=torch.zeros((W, 2), dtype=torch.int64),
                response=torch.zeros(W, dtype=torch.int64), out=torch.zeros((W, CH, FRAMES), dtype=torch.float16),
                gain=torch.ones(W, dtype=torch.float32), spans=torch.zeros((W, 2), dtype=torch.int64))
    return plan, conv, good


def test_convolver_create_hands_over_taps_lengths_and_delays(engine):
    _setup(engine)
    args = engine.lib.last("AADHip_ConvolverCreate")
    assert args[1] == 2 and list(args[3]) == [1, 3] and list(args[4]) == [-1, 2]
    assert np.frombuffer(C.string_at(args[2][1], 12), dtype=np.float32).tolist() == [0.5, 0.25, -0.125]
    engine.convolver([[1.0]])
    assert engine.lib.last("AADHip_ConvolverCreate")[4] is None
    before = len(engine.lib.calls)
    for bad in ([], [[]], [np.zeros(32769)]):
        with pytest.raises(ValueError, match="responses"):
            engine.convolver(bad)
    for bad in ([0], [0, 3], [0, -2]):
        with pytest.raises(ValueError, match="delays"):
            engine.convolver([[1.0], [0.5, 0.25, -0.125]], delays=bad)
    assert engine.lib.calls[before:] == []


def test_run_is_resolve_window_decode_fir_in_that_order(engine):
    plan, conv, good = _setup(engine)
    before = len(engine.lib.calls)
    out = conv.run(plan, good["data"], good["windows"], FRAMES, response=good["response"], dtype=torch.float16, out=good["out"])
    assert out is good["out"]
    names = [c[0] for c in engine.lib.calls[before:]]
    assert names == ["AADHip_ConvolverSourceFrames", "AADHip_ConvolverResolve", "AADHip_WindowDecodePlanRun", "AADHip_ConvolverRun"]
    resolve = engine.lib.last("AADHip_ConvolverResolve")
    assert list(resolve[:5]) == [conv.handle, W, good["windows"].data_ptr(), good["response"].data_ptr(), FRAMES]
    decode = engine.lib.last("AADHip_WindowDecodePlanRun")
    assert list(decode[:6]) == [plan.handle, good["data"].data_ptr(), W, resolve[5], T_SRC, capi.SAMPLE_INT16]
    run = engine.lib.last("AADHip_ConvolverRun")
    assert list(run) == [conv.handle, W, CH, decode[6], T_SRC, resolve[6], FRAMES, capi.SAMPLE_FLOAT16, good["out"].data_ptr()]
    # no response table: NULL; no out: allocated, float32
    out = conv.run(plan, good["data"], good["windows"], FRAMES)
    assert engine.lib.last("AADHip_ConvolverResolve")[3] is None
    assert out.dtype == torch.float32 and tuple(out.shape) == (W, CH, FRAMES)
    # gain, accumulate and spans go to the gain run
    conv.run(plan, good["data"], good["windows"], FRAMES, dtype=torch.float16, out=good["out"], gain=good["gain"], accumulate=True,
             spans=good["spans"])
    gain = engine.lib.last("AADHip_ConvolverRunGain")
    assert gain[6] == good["spans"].data_ptr() and gain[7:] == (FRAMES, capi.SAMPLE_FLOAT16, good["out"].data_ptr(), good["gain"].data_ptr(),
                                                                 capi.WINDOW_GAIN_ADD)
    conv.run(plan, good["data"], good["windows"], FRAMES, spans=good["spans"])
    assert engine.lib.last("AADHip_ConvolverRunGain")[6] == good["spans"].data_ptr() and engine.lib.last("AADHip_ConvolverRunGain")[10:] == \
        (None, capi.WINDOW_GAIN_STORE)
    conv.close()
    assert engine.lib.calls[-1][0] == "AADHip_ConvolverDestroy" and conv.handle is None


REFUSALS = [
    ("windows", lambda g: g["windows"].to(torch.int32), "windows: dtype"),
    ("windows", lambda g: torch.zeros((W, 3), dtype=torch.int64), "windows: shape"),
    ("windows", lambda g: torch.zeros((W, 2), dtype=torch.int64, device="meta"), "windows: a tensor on the engine's device"),
    ("response", lambda g: g["response"].to(torch.int32), "response: dtype"),
    ("response", lambda g: torch.zeros(W + 1, dtype=torch.int64), "response: shape"),
    ("response", lambda g: torch.zeros(2 * W, dtype=torch.int64)[::2], "response: a contiguous tensor"),
    ("response", lambda g: torch.zeros(W, dtype=torch.int64, device="meta"), "response: a tensor on the engine's device"),
    ("out", lambda g: g["out"].to(torch.float32), "out: dtype"),
    ("out", lambda g: torch.zeros((W, CH, FRAMES + 1), dtype=torch.float16), "out: shape"),
    ("out", lambda g: torch.zeros((W, CH, FRAMES + 3), dtype=torch.float16)[..., :FRAMES], "out: a contiguous tensor"),
    ("out", lambda g: torch.zeros((W, CH, FRAMES), dtype=torch.float16, device="meta"), "out: a tensor on the engine's device"),
    ("gain", lambda g: g["gain"].to(torch.float64), "gain: dtype"),
    ("gain", lambda g: torch.ones(W + 1, dtype=torch.float32), "gain: shape"),
    ("gain", lambda g: torch.ones(2 * W, dtype=torch.float32)[::2], "gain: a contiguous tensor"),
    ("spans", lambda g: g["spans"].to(torch.int32), "spans: dtype"),
    ("spans", lambda g: torch.zeros((W + 1, 2), dtype=torch.int64), "spans: shape"),
]


@pytest.mark.parametrize("name,spoil,message", REFUSALS, ids=[r[2].replace(": ", "-").replace(" ", "_") for r in REFUSALS])
def test_run_refuses_a_tensor_off_its_contract(engine, name, spoil, message):
    plan, conv, good = _setup(engine)
    before = len(engine.lib.calls)
    bad = dict(good, **{name: spoil(good)})
    with pytest.raises(ValueError, match=message):
        conv.run(plan, bad["data"], bad["windows"], FRAMES, response=bad["response"], dtype=torch.float16, out=bad["out"], gain=bad["gain"],
                 spans=bad["spans"])
    assert engine.lib.calls[before:] == []  # nothing reached the library


def test_run_refuses_what_the_gain_run_cannot_do(engine):
    plan, conv, good = _setup(engine)
    before = len(engine.lib.calls)
    with pytest.raises(ValueError, match="convolve writes"):
        conv.run(plan, good["data"], good["windows"], FRAMES, dtype=torch.float64)
    with pytest.raises(ValueError, match="float rows only"):
        conv.run(plan, good["data"], good["windows"], FRAMES, dtype=torch.int16, gain=good["gain"])
    with pytest.raises(ValueError, match="float rows only"):
        conv.run(plan, good["data"], good["windows"], FRAMES, dtype=torch.int16, spans=good["spans"])
    with pytest.raises(ValueError, match="accumulate=True adds into `out`"):
        conv.run(plan, good["data"], good["windows"], FRAMES, accumulate=True)
    assert engine.lib.calls[before:] == []


def test_run_source_holds_the_record_to_its_shape(engine):
    plan, conv, good = _setup(engine)
    rows = torch.zeros((W, CH, T_SRC), dtype=torch.int16)
    lanes = torch.zeros((W, 2), dtype=torch.int32)
    out = conv.run_source(ConvolveSource(rows, lanes, T_SRC), FRAMES, CH)
    run = engine.lib.last("AADHip_ConvolverRun")
    assert list(run) == [conv.handle, W, CH, rows.data_ptr(), T_SRC, lanes.data_ptr(), FRAMES, capi.SAMPLE_FLOAT32, out.data_ptr()]
    before = len(engine.lib.runs()) + sum(c[0].startswith("AADHip_ConvolverRun") for c in engine.lib.calls)
    for source, message in ((ConvolveSource(rows, lanes.to(torch.int64), T_SRC), "source.lanes: dtype"),
                            (ConvolveSource(rows, torch.zeros((W, 3), dtype=torch.int32), T_SRC), "source.lanes: shape"),
                            (ConvolveSource(rows.to(torch.float32), lanes, T_SRC), "source.rows: dtype"),
                            (ConvolveSource(rows[:, :, :T_SRC - 1], lanes, T_SRC), "source.rows: shape"),
                            (ConvolveSource(rows, lanes, T_SRC + 1), "source.rows: shape"),
                            (ConvolveSource(rows[:, :, :T_SRC - 1].contiguous(), lanes, T_SRC - 1), "source.rows: 998 frames")):
        with pytest.raises(ValueError, match=message):
            conv.run_source(source, FRAMES, CH)
    assert len(engine.lib.runs()) + sum(c[0].startswith("AADHip_ConvolverRun") for c in engine.lib.calls) == before


def test_decode_windows_reverberated_builds_convolver_and_plan(engine):
    from test_engine_tensor_contract import header_bytes
    data = torch.zeros((3, 64), dtype=torch.uint8)
    data[:, :31] = torch.frombuffer(bytearray(header_bytes(CH, 100)), dtype=torch.uint8)
    windows = torch.zeros((W, 2), dtype=torch.int64)
    out = engine.decode_windows_reverberated(data, 64, windows, FRAMES, [[1.0], [0.25, 0.5]], response=torch.zeros(W, dtype=torch.int64))
    assert tuple(out.shape) == (W, CH, FRAMES) and out.dtype == torch.float32
    names = [c[0] for c in engine.lib.calls]
    assert names.index("AADHip_ConvolverCreate") < names.index("AADHip_ConvolverResolve") < names.index("AADHip_WindowDecodePlanRun") \
        < names.index("AADHip_ConvolverRun")
    assert names[-2:] == ["AADHip_ConvolverDestroy", "AADHip_WindowDecodePlanDestroy"]
    # a refused argument is found before the convolver is built
    before = len(engine.lib.calls)
    for bad, message in ((dict(windows=windows.to(torch.int32)), "windows: dtype"), (dict(response=torch.zeros(W + 1, dtype=torch.int64)), "response: shape"),
                         (dict(out=torch.zeros((W, CH, FRAMES + 1))), "out: shape"), (dict(gain=torch.ones(W + 1)), "gain: shape"),
                         (dict(dtype=torch.int16, spans=torch.zeros((W, 2), dtype=torch.int64)), "float rows only"),
                         (dict(dtype=torch.float64), "convolve writes"), (dict(responses=[[]]), "responses"), (dict(delays=[3]), "delays")):
        args = dict(dict(windows=windows, responses=[[1.0]]), **bad)
        with pytest.raises(ValueError, match=message):
            engine.decode_windows_reverberated(data, 64, args.pop("windows"), FRAMES, args.pop("responses"), **args)
    assert not any(c[0].startswith("AADHip_Convolver") for c in engine.lib.calls[before:])
