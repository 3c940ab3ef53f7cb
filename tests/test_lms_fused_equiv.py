"""The quad mapping updates a tap's weight with one 64-bit multiply-add whose addend carries the weight in its
upper dword (aad_amd/csrc/aad_device.hip.h lms_first_fused).  tests/lms_fused_equiv.c proves it equal to the
reference's int32 update for every dequantised difference in [-65536, 65535] and every int16 history sample, and
for weights at the int32 rails; the GPU side of the same claim is tests/test_gpu_quad_lms.py.

The reference's own expression overflows int32 for one of the 2^33 pairs, qd = -65536 with h = -32768 (undefined
in C; no coder reaches it, |qd| <= 61438).  The program checks that this is the only such pair and that the device
form gives the exact value there; the other 2^33 - 1 pairs must agree."""
import hashlib
import os
import struct
import subprocess


def test_fused_tap_update_equals_reference(tmp_path):
    src = os.path.join(os.path.dirname(__file__), "lms_fused_equiv.c")
    exe = tmp_path / "lfe"
    subprocess.run(["gcc", "-O3", "-fwrapv", "-pthread", "-o", str(exe), src], check=True)
    weights = [0, 1, -1, 1 << 30, -(1 << 30), 2**31 - 1, -(2**31)]
    weights += list(struct.unpack("<1024i", hashlib.shake_256(b"lms_fused_equiv weights").digest(4096)))
    wfile = tmp_path / "weights.txt"
    wfile.write_text("\n".join(str(w) for w in weights) + "\n")
    out = subprocess.run([str(exe), str(wfile)], check=True, capture_output=True, text=True).stdout.split()
    checked, bad, overflowed, wchecked, wbad = (int(v) for v in out)
    assert checked == 1 << 33 and bad == 0
    assert overflowed == 1  # qd = -65536, h = -32768: the reference's product is 2^31
    qds, hs = 7 + len(range(-65536 + 3, 65536, 509)), 5 + len(range(-32768 + 5, 32768, 127))
    assert wchecked == len(weights) * (qds * hs - 1) and wbad == 0
