"""Planar encode on the CPU: the float32 -> int16 rule the encoder kernels apply to planar float32 input
(aad_amd/csrc/aad_pcm_convert.h, include/aad_hip.h "planar encode") and the planar chain table of segmented plans
(aad_amd/csrc/aad_segments.h), through tests/planar_host_driver.cpp built with g++ against those same headers.

  * pcm_from_f32 equals a plain C statement of q (double arithmetic, the tie rule written out) on all 2^32 float32 bit patterns;
  * it equals torch's nan_to_num(x, nan=0).mul(32768).round().clamp(-32768, 32767).to(int16) on the special values and a
    random sample of bit patterns;
  * a planar chain starts first_frame elements into channel 0's row (interleaved: first_frame * channels int16 into the
    stream); every other field of the table is the interleaved one."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aad_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("planar") / "planar_host_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-pthread", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "planar_host_driver.cpp")],
                   check=True)
    return str(exe)


def special_values():
    """the values include/aad_hip.h's rule has to get right, as float32"""
    f = np.float32
    ties = [(k + 0.5) / 32768 for k in range(-32770, -32760)] + [(k + 0.5) / 32768 for k in range(-6, 6)] + \
           [(k + 0.5) / 32768 for k in range(32760, 32770)]
    vals = [0.0, -0.0, 1.0, -1.0, 32767 / 32768, -32767 / 32768, 32768 / 32768, -32769 / 32768, 0.5 / 32768, -0.5 / 32768,
            1e-30, -1e-30, 3e38, -3e38, 65504.0, -65504.0, 1e10, -1e10, np.inf, -np.inf] + ties
    x = np.array(vals, dtype=np.float64).astype(f)
    bits = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0x7FFFFFFF,  # quiet and signalling NaNs
            0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,  # denormals, smallest normals
            0x7F7FFFFF, 0xFF7FFFFF]                                                  # largest finite
    x = np.concatenate([x, np.array(bits, dtype=np.uint32).view(f)])
    # every float32 next to the clamp bounds and the ties
    near = np.array([32767 / 32768, -1.0, 0.5 / 32768, 1.5 / 32768, -0.5 / 32768, 32766.5 / 32768], dtype=f)
    steps = np.concatenate([near.view(np.uint32) + np.uint32(d) for d in range(0, 4)] +
                           [near.view(np.uint32) - np.uint32(d) for d in range(1, 4)]).view(f)
    return np.concatenate([x, steps])


def torch_q(x):
    import torch
    t = torch.from_numpy(x.copy())
    return torch.nan_to_num(t, nan=0.0).mul(32768).round().clamp(-32768, 32767).to(torch.int16).numpy().astype(np.int32)


def driver_q(driver, x, tmp_path):
    src, dst = tmp_path / "in.f32", tmp_path / "out.i32"
    np.ascontiguousarray(x, dtype="<f4").tofile(str(src))
    subprocess.run([driver, "convert", str(src), str(dst)], check=True)
    return np.fromfile(str(dst), dtype="<i4")


def test_conversion_over_every_float32_bit_pattern(driver):
    out = subprocess.run([driver, "exhaustive"], check=True, capture_output=True, text=True, timeout=1200).stdout.split()
    assert out[0] == "mismatches" and out[1] == "0", "pcm_from_f32 differs from q at bit pattern 0x%s (%s mismatches)" % (out[2], out[1])


def test_conversion_matches_torch_on_specials_and_random_bit_patterns(driver, tmp_path):
    rng = np.random.default_rng(2026)
    x = np.concatenate([special_values(), rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        rng.uniform(-1.5, 1.5, size=1 << 18).astype(np.float32)])
    got, want = driver_q(driver, x, tmp_path), torch_q(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first mismatch: bits 0x%08x -> %d, torch %d" % (x[bad[0]:bad[0] + 1].view(np.uint32)[0], got[bad[0]], want[bad[0]])


def test_conversion_fixed_points(driver, tmp_path):
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, -1.0, 0.5 / 32768, 1.5 / 32768, -0.5 / 32768, -1.5 / 32768, 32767.5 / 32768],
                 dtype=np.float32)
    assert driver_q(driver, x, tmp_path).tolist() == [0, 32767, -32768, 0, 32767, -32768, 0, 2, 0, -2, 32767]


def chain_table(driver, planar, channels, spb, block_size, L, W, streams):
    lines = ["%d %d %d %d %d %d" % (channels, spb, block_size, L, W, len(streams))]
    lines += ["%d %d %d" % s for s in streams]
    out = subprocess.run([driver, "chains", "1" if planar else "0"], input="\n".join(lines) + "\n", check=True, capture_output=True,
                         text=True).stdout.strip().split("\n")
    assert out[0].startswith("ok ")
    return [tuple(int(v) for v in line.split()) for line in out[1:]]


def test_planar_chains_start_inside_channel_0_row(driver):
    # 2 channels, 100 frames per block, L = 2, W = 1: a stream of 450 frames has 5 blocks -> segments {0, 1}, {2, 3}, {4}
    streams = [(1000, 0, 450), (1 << 40, 4096, 99)]
    planar = chain_table(driver, True, 2, 100, 436, 2, 1, streams)
    inter = chain_table(driver, False, 2, 100, 436, 2, 1, streams)
    assert [c[0] for c in planar] == [1000, 1100, 1300, 1 << 40]
    assert [c[0] for c in inter] == [1000, 1200, 1600, 1 << 40]
    assert [c[1:] for c in planar] == [c[1:] for c in inter]


@pytest.mark.parametrize("channels", [1, 3, 8])
def test_planar_chains_other_channel_counts(driver, channels):
    streams = [(7, 0, 1000), (123457, 9999, 2048)]
    planar = chain_table(driver, True, channels, 64, 1024, 3, 1, streams)
    inter = chain_table(driver, False, channels, 64, 1024, 3, 1, streams)
    assert len(planar) == len(inter)
    for p, i in zip(planar, inter):
        base = 7 if p[1] == 0 else 123457
        assert p[0] - base == (i[0] - base) // channels and p[1:] == i[1:]
