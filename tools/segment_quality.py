"""Quality cost of a segmented encode (AADHip_SegmentedEncodePlanCreate), on the CPU with the oracle: for each point of a grid of
(bits, trials, L, W), the RMSE of the decoded segmented image over the RMSE of the decoded serial encode (both against the input, as
`aad -c` computes RMSE), and how many segments came out byte-identical to the serial encode's blocks.  The numbers are
deterministic.  CPU only by default: it then never touches the GPU, and bench.py, smoke() and the GPU tests do not use it.
--device adds a column with the same ratio taken on the device from exact integer sums (Engine.codec_error on the segmented and on
the serial plan: sqrt of the quotient of the squared-error sums over all channels); the CPU columns stay as they are.

    python tools/segment_quality.py WAV [WAV ...] [--bits 4,2] [--trials 0,2] [--L 16,64,128,256] [--W 0,8,16,32,64]
                                    [--max-block-size 1024] [--out FILE] [--device]

The image of a segmented encode is defined in include/aad_hip.h; tests/segment_oracle.py builds it from the definition."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import oracle_binding as ob  # noqa: E402
import segment_oracle as so  # noqa: E402
from helpers import read_wav16  # noqa: E402


def ints(s):
    return [int(v) for v in s.split(",") if v != ""]


def identical_segments(serial, image, block_size, spb, frames, L):
    """segments whose blocks (file header excluded) are the serial encode's bytes"""
    count = 0
    for s in range(len(so.segments(frames, spb, L, 0))):
        a = 31 + s * L * block_size
        b = 31 + (s + 1) * L * block_size
        count += serial[a:b] == image[a:b]
    return count


def device_sum_sq(engine, x, param, L=None, W=0):
    """the squared codec error of x ([1, C, T] int16 on the device) summed over its channels, as a Python int"""
    return int(engine.codec_error(x, param, segment_blocks=L, warmup_blocks=W)[..., 0].sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("wavs", nargs="+")
    ap.add_argument("--bits", type=ints, default=[4, 2])
    ap.add_argument("--trials", type=ints, default=[0, 2])
    ap.add_argument("--L", type=ints, default=[16, 64, 128, 256])
    ap.add_argument("--W", type=ints, default=[0, 8, 16, 32, 64])
    ap.add_argument("--max-block-size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", action="store_true", help="add the RMSE ratio measured on the device (Engine.codec_error)")
    args = ap.parse_args()
    engine = None
    if args.device:
        import torch
        from aad_amd.capi import make_parameter
        from aad_amd.engine import Engine
        engine = Engine(0)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libaad_oracle.so"], check=True)
    mbs = args.max_block_size
    lines = ["# segmented encode quality: RMSE(decoded segmented image) / RMSE(decoded serial encode), both against the input",
             "# (RMSE as `aad -c` prints it); identical = segments byte-identical to the serial encode's blocks; max block size %d" % mbs,
             "%-18s %4s %6s %5s %4s %4s %8s %12s %12s %9s" % ("file", "bits", "trials", "L", "W", "segs", "blocks", "rmse_serial",
                                                             "rmse_seg", "ratio") + "  identical" + ("  dev_ratio" if engine else "")]
    print("\n".join(lines), flush=True)
    for path in args.wavs:
        pcm, rate = read_wav16(path)
        frames, ch = pcm.shape
        for bits in args.bits:
            _, block_size, spb = ob.geometry(mbs, ch, bits)
            blocks = -(-frames // spb)
            for trials in args.trials:
                serial = ob.encode(pcm, bits, mbs, rate, False, trials)
                rmse_serial = ob.error_stats(pcm, ob.decode(serial)[0])[0]
                if engine:
                    x = torch.from_numpy(pcm.T.copy()).cuda()[None]
                    param = make_parameter(ch, bits, mbs, rate, False, trials)
                    dev_serial = device_sum_sq(engine, x, param)
                for L in args.L:
                    segs = -(-blocks // L)
                    for W in args.W:
                        img = so.segmented_encode(pcm, bits, L, W, mbs, rate=rate, trials=trials)
                        rmse = ob.error_stats(pcm, ob.decode(img)[0])[0]
                        row = "%-18s %4d %6d %5d %4d %4d %8d %12.6f %12.6f %9.4f  %d" % (
                            os.path.basename(path), bits, trials, L, W, segs, blocks, rmse_serial, rmse,
                            rmse / rmse_serial if rmse_serial else float("nan"),
                            identical_segments(serial, img, block_size, spb, frames, L))
                        if engine:
                            dev = device_sum_sq(engine, x, param, L, W)
                            row += "  %9.4f" % ((dev / dev_serial) ** 0.5 if dev_serial else float("nan"))
                        print(row, flush=True)
                        lines.append(row)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if engine:
        engine.close()


if __name__ == "__main__":
    main()
