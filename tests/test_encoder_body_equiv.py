"""The quad encoder's chunk body dequantises, applies the sign and reconstructs in one 64-bit
multiply-add (aad_amd/csrc/aad_encode.hip.h encode_chunk16_quad).  tests/encoder_body_equiv.c proves
it equal to the reference's formula for every step, magnitude, sign, bit width and prediction; the
GPU side of the same claim is covered by the parity tests."""
import os
import subprocess


def test_fused_dequantiser_equals_reference(tmp_path):
    src = os.path.join(os.path.dirname(__file__), "encoder_body_equiv.c")
    exe = tmp_path / "ebe"
    subprocess.run(["gcc", "-O2", "-fwrapv", "-o", str(exe), src], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    # bits 2, 3, 4: magnitudes 0..1, 0..3, 0..7; two signs; 131072 predictions
    assert int(out[0]) == 256 * (2 + 4 + 8) * 2 * 131072 and int(out[1]) == 0
