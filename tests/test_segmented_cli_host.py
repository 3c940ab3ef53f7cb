"""Segmented encode on the host side, without a GPU: aad_batch's -S / --segment-blocks option (help line, usage errors), and the waves
of the host-memory path (aad_amd/csrc/aad_segments.h build_segment_waves), printed by tests/segment_waves_driver.cpp built with g++.

The wave checks restate what the kernel does with a chain record (aad_encode.hip.h, SEG): it stores the file header at data_offset
(writes_header only) and kept block i at data_offset + 31 + (first_block + warmup_blocks + i) * block_size.  Every block of every stream
must be stored by exactly one chain across the waves of a batch, land where the wave's delivery of that chain expects it, and the
chain's frames must be the definition's (include/aad_hip.h, above struct AADHipSegmentation)."""
import os
import subprocess

import pytest

from helpers import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "aad_amd", "csrc")
CLI = os.path.join(ROOT, "aad_amd", "aad_batch")
HEADER = 31


def _run(args):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


# ---- aad_batch -S --------------------------------------------------------------------------------------------------------------

def test_help_lists_segment_blocks():
    r = _run(["-h"])
    assert r.returncode == 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("  -")]
    seg = [l for l in lines if "--segment-blocks" in l]
    assert len(seg) == 1 and seg[0].startswith("  -S, --segment-blocks") and "(needs argument)" in seg[0]
    # behind the reference's table and this front end's other options
    assert lines.index(seg[0]) > max(i for i, l in enumerate(lines) if "--devices" in l)


@pytest.mark.parametrize("value", ["0", "0,4", "abc", "4x", "4,", "4,x", "4,2,1", ",3", "-4", " 4", "+4", "4,-1", "",
                                   "4294967296", "4,4294967296"])
def test_segment_blocks_usage_errors(tmp_path, value):
    # these alone do not prove the parser (an unknown option is a usage error too):
    # test_segment_blocks_accepted_forms_reach_the_inputs shows that well-formed values are taken
    for mode in (["-e", "-o", str(tmp_path)], ["-r", "-o", str(tmp_path)], ["-g", "-o", str(tmp_path)], ["-c"]):
        for flag in ("-S", "--segment-blocks"):
            r = _run(mode + [flag, value, str(tmp_path / "x.wav")])
            assert r.returncode == 2 and "usage:" in r.stderr, (mode, flag, value, r.stderr)


def test_segment_blocks_with_decode_or_information_is_a_usage_error(tmp_path):
    assert _run(["-d", "-o", str(tmp_path), "-S", "4", str(tmp_path / "x.aad")]).returncode == 2
    assert _run(["-d", "-S", "4,2", "-o", str(tmp_path), str(tmp_path / "x.aad")]).returncode == 2
    assert _run(["-i", "-S", "4", str(tmp_path / "x.aad")]).returncode == 2
    assert _run(["-e", "-o", str(tmp_path), str(tmp_path / "x.wav"), "-S"]).returncode == 2  # no value


def test_segment_blocks_accepted_forms_reach_the_inputs(tmp_path):
    """well-formed values pass the parser: the run then fails on the missing input (1), not on usage (2)"""
    missing = str(tmp_path / "missing.wav")
    for value in ("1", "4", "64,8", "256,32", "4294967295,4294967295", "7,0"):
        for mode in (["-e", "-o", str(tmp_path)], ["-r", "-o", str(tmp_path)], ["-g", "-o", str(tmp_path)], ["-c"]):
            r = _run(mode + ["--segment-blocks", value, missing])
            assert r.returncode == 1 and "cannot read" in r.stderr, (mode, value, r.returncode, r.stderr)
    assert _run(["-h", "-S", "0"]).returncode == 0  # help still wins over everything else


# ---- waves of the host-memory path -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("waves") / "segment_waves_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(HERE, "segment_waves_driver.cpp")], check=True)
    return str(exe)


def image_size(n, ch, spb, bs):
    """a stand-in for AADFormat_EncodedSize: whole blocks of bs bytes, a shorter last one"""
    full, tail = divmod(n, spb)
    return HEADER + full * bs + (min(bs - 1, 4 * ch + (tail * ch + 1) // 2) if tail else 0)


def waves(driver, ch, spb, bs, L, W, budget, samples):
    sizes = [image_size(n, ch, spb, bs) for n in samples]
    text = "%d %d %d %d %d %d %d\n" % (ch, spb, bs, L, W, budget, len(samples))
    text += "".join("%d %d\n" % (n, s) for n, s in zip(samples, sizes))
    out = subprocess.run([driver], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    if out[0] == "refused":
        return None, sizes
    count = int(out[0].split()[1])
    result, at = [], 1
    for _ in range(count):
        _, n, pcm_elems, out_begin, out_bytes = out[at].split()
        keys = ("stream frame0 image_offset image_bytes out_offset pcm_offset data_offset first_block num_frames warmup_blocks "
                "header_samples writes_header").split()
        chains = [dict(zip(keys, (int(v) for v in out[at + 1 + k].split()))) for k in range(int(n))]
        result.append(dict(pcm_elems=int(pcm_elems), out_begin=int(out_begin), out_bytes=int(out_bytes), chains=chains))
        at += 1 + int(n)
    return result, sizes


def chain_cost(c, ch):
    return (c["num_frames"] * ch + 7) // 8 * 8 * 2 + (c["image_bytes"] + 15) // 16 * 16


def check_batch(driver, ch, spb, bs, L, W, budget, samples):
    """every invariant of the waves of one batch; returns them"""
    result, sizes = waves(driver, ch, spb, bs, L, W, budget, samples)
    assert result is not None
    blocks = [max(1, -(-n // spb)) for n in samples]
    written = [[0] * b for b in blocks]                  # chains that store each block
    delivered = [bytearray(s) for s in sizes]            # deliveries that cover each image byte
    order = []
    for t in result:
        assert t["chains"], "an empty wave"
        pcm_used, out_used = [], []
        for c in t["chains"]:
            i, n, w = c["stream"], samples[c["stream"]], c["warmup_blocks"]
            order.append(i)
            assert c["header_samples"] == n and c["first_block"] == 0
            # the chain's frames: the definition's slice of its stream
            kept = (c["frame0"] // spb) + w
            assert c["frame0"] == (kept - w) * spb and kept % L == 0 and w == min(W, kept)
            assert c["frame0"] + c["num_frames"] == min((kept + L) * spb, n)
            nk = -(-(c["num_frames"] - w * spb) // spb) if n else 1
            assert 1 <= nk <= L
            assert c["writes_header"] == (kept == 0)
            # where the kernel stores, in the wave's output block, and where the delivery takes the bytes from
            if c["writes_header"]:
                assert c["data_offset"] == c["out_offset"] and c["image_offset"] == 0
            else:
                assert c["data_offset"] + HEADER + w * bs == c["out_offset"]  # no wrap: data_offset <= out_offset
                assert c["image_offset"] == HEADER + kept * bs
            end = min(HEADER + (kept + nk) * bs, sizes[i])
            assert c["image_offset"] + c["image_bytes"] == end
            for j in range(nk):
                store = c["data_offset"] + HEADER + (c["first_block"] + w + j) * bs
                assert store - c["out_offset"] == HEADER + (kept + j) * bs - c["image_offset"]
                written[i][kept + j] += 1
            for b in range(c["image_offset"], end):
                delivered[i][b] += 1
            assert c["out_offset"] >= t["out_begin"] and c["out_offset"] + c["image_bytes"] <= t["out_bytes"]
            assert c["pcm_offset"] % 8 == 0 and c["pcm_offset"] + c["num_frames"] * ch <= t["pcm_elems"]
            pcm_used.append((c["pcm_offset"], c["pcm_offset"] + c["num_frames"] * ch))
            out_used.append((c["out_offset"], c["out_offset"] + c["image_bytes"]))
        for used in (pcm_used, out_used):
            used.sort()
            assert all(a[1] <= b[0] for a, b in zip(used, used[1:])), "chains of a wave overlap"
        assert t["out_begin"] % 16 == 0 and t["out_begin"] <= HEADER + W * bs + 15
        cost = sum(chain_cost(c, ch) for c in t["chains"])
        assert len(t["chains"]) == 1 or cost <= budget
    assert all(all(k == 1 for k in s) for s in written), "a block stored by no chain or by several"
    assert all(all(k == 1 for k in d) for d in delivered), "an image byte delivered by no chain or by several"
    assert order == sorted(order), "chains leave the batch's order"
    for a, b in zip(result, result[1:]):  # greedy: the next wave's first chain did not fit
        assert sum(chain_cost(c, ch) for c in a["chains"]) + chain_cost(b["chains"][0], ch) > budget
    return result


def test_one_wave_when_the_budget_covers_the_batch(driver):
    t = check_batch(driver, 2, 10, 40, 3, 2, 1 << 40, [95, 7, 10, 300])
    assert len(t) == 1 and len(t[0]["chains"]) == 4 + 1 + 1 + 10


@pytest.mark.parametrize("budget", [1, 100, 700, 1500, 4000, 20000])
@pytest.mark.parametrize("L,W", [(1, 0), (1, 3), (3, 5), (4, 0), (7, 2), (64, 8), (2, 1000)])
def test_every_block_written_once_under_small_budgets(driver, L, W, budget):
    samples = [1, 9, 10, 11, 95, 400, 1003, 3, 250]
    t = check_batch(driver, 2, 10, 40, L, W, budget, samples)
    if budget <= 700:
        # a long stream spreads its chains over several waves, and waves cut between chains of one stream
        spans = {}
        for k, wave in enumerate(t):
            for c in wave["chains"]:
                spans.setdefault(c["stream"], set()).add(k)
        assert max(len(v) for v in spans.values()) > 1 or max(-(-n // 10) for n in samples) <= L


def test_a_chain_larger_than_the_budget_is_a_wave_of_its_own(driver):
    # one 50-block segment costs far more than 512 bytes: every wave holds exactly one chain
    t = check_batch(driver, 1, 16, 36, 50, 4, 512, [16 * 200 - 5, 16 * 50, 7])
    assert [len(x["chains"]) for x in t] == [1] * len(t) and len(t) == 4 + 1 + 1
    assert all(chain_cost(x["chains"][0], 1) > 512 for x in t[:5])


def test_a_long_stream_among_many_short_ones(driver):
    samples = [5, 17] * 40 + [10 * 900 + 3] + [12] * 40
    for budget in (300, 2000, 9000):
        t = check_batch(driver, 2, 10, 40, 16, 4, budget, samples)
        assert len(t) > 1


def test_eight_channels_and_the_warmup_clamped_at_the_stream_start(driver):
    check_batch(driver, 8, 10, 200, 2, 5, 3000, [50, 10, 1, 203])


def test_refused_above_uint32_max_chains(driver):
    assert waves(driver, 1, 4, 20, 1, 0, 1 << 20, [0xFFFFFFFF] * 4)[0] is None
    assert waves(driver, 1, 4, 20, 0, 0, 1 << 20, [100])[0] is None
