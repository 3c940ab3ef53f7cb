"""Expected bytes of a segmented encode (AADHip_SegmentedEncodePlanCreate, include/aad_hip.h), built from the definition: per
segment a fresh encoder over the segment's frames with its warm-up in front, the warm-up blocks dropped, the stream's file header
in front of all.  TESTS AND TOOLS ONLY (pinned by tests/test_segment_definition.py)."""
import ctypes as C
import os

import numpy as np

import oracle_binding as ob


def oracle_encoder(bits, max_block_size=1024, rate=48000, ms=False, trials=0):
    """encode(pcm int16 [frames, channels]) -> bytes, by the oracle (every channel count, M/S, any trial count)"""
    return lambda pcm: ob.encode(pcm, bits, max_block_size, rate, ms, trials)


_ref = None


def ref_lib():
    global _ref
    if _ref is None:
        r = C.CDLL(ob.REF_SO)
        r.refbatch_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_size_t, C.c_void_p]
        r.refbatch_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        _ref = r
    return _ref


def ref_encoder(bits, max_block_size=1024, trials=0):
    """the compiled reference's AADEncoder_EncodeWhole (oracle/_ref, L/R at 48 kHz: what refbatch_encode sets)"""
    def enc(pcm):
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        n, ch = pcm.shape
        planar = np.ascontiguousarray(pcm.T, dtype=np.int32)
        cap = ob.encoded_size(n, ch, bits, max_block_size) + 64
        out = np.zeros(cap, dtype=np.uint8)
        size = np.zeros(1, dtype=np.uint32)
        rc = ref_lib().refbatch_encode(planar.ctypes.data, 1, n, ch, bits, max_block_size, trials, out.ctypes.data, cap,
                                       size.ctypes.data)
        assert rc == 0, "reference encode rc=%d" % rc
        return out[:size[0]].tobytes()
    return enc


def ref_decode(image, num_samples, channels):
    """the compiled reference's AADDecoder_DecodeWhole -> int16 [frames, channels]"""
    buf = np.frombuffer(image, dtype=np.uint8).copy()
    planar = np.zeros((channels, num_samples), dtype=np.int32)
    sizes = np.array([len(buf)], dtype=np.uint32)
    rc = ref_lib().refbatch_decode(buf.ctypes.data, 1, len(buf), sizes.ctypes.data, num_samples, channels, planar.ctypes.data)
    assert rc == 0, "reference decode rc=%d" % rc
    return np.ascontiguousarray(planar.T).astype(np.int16)


def segments(num_frames, spb, segment_blocks, warmup_blocks):
    """[(first encoded frame, end frame, warm-up blocks)] of a stream, segment by segment"""
    blocks = max(1, -(-num_frames // spb))
    out = []
    for s in range(-(-blocks // segment_blocks)):
        kept = s * segment_blocks
        w = min(warmup_blocks, kept)
        out.append(((kept - w) * spb, min((s + 1) * segment_blocks * spb, num_frames), w))
    return out


def segmented_encode(pcm, bits, segment_blocks, warmup_blocks, max_block_size=1024, encode=None, **kw):
    """The image of one stream (int16 [frames, channels]) by the definition; `encode` encodes a slice with a fresh encoder
    (default: the oracle with the keyword arguments rate / ms / trials)."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    n, ch = pcm.shape
    if encode is None:
        encode = oracle_encoder(bits, max_block_size, **kw)
    rc, block_size, spb = ob.geometry(max_block_size, ch, bits)
    assert rc == 0
    parts = []
    for i, (f0, f1, w) in enumerate(segments(n, spb, segment_blocks, warmup_blocks)):
        img = encode(pcm[f0:f1])
        if i == 0:
            head = bytearray(img[:31])
            head[14:18] = n.to_bytes(4, "big")  # the stream's num_samples (big-endian, bytes 14..17)
            parts.append(bytes(head))
        parts.append(img[31 + w * block_size:])
    return b"".join(parts)
