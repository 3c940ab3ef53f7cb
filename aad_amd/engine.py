"""Python mirror of the batched C-ABI (include/aad_hip.h).

torch is plumbing only: it owns the device tensors and the stream that are handed to the C
library as raw pointers.  All codec work happens in libaad_hip.so's HIP kernels; if the library
or a GPU is missing every call here raises - there is no fallback path.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from .capi import (AADApiResult, AADHeaderInfo, AADHipResampleRatio, RESAMPLE_NO_BANK, AADHipPlanarLayout, AADHipPlanarOutput, AADHipSegmentation, ApiError, ERROR_STATS_DTYPE, LANE_MAPPINGS, LANE_STATE_DTYPE,
                   OPTION_COMPARE_ORDER, OPTION_LANE_MAPPING, OPTION_SIMD_ROLE, OPTION_STAGING_THREADS, OPTION_TILE_KBYTES, OPTION_TRIAL_LANES, RECONSTRUCT_DECODED, RECONSTRUCT_RESIDUAL,
                   SAMPLE_BFLOAT16, SAMPLE_FLOAT16, SAMPLE_FLOAT32, SAMPLE_INT16, SIMD_ROLE_OFF, STREAM_DESC_DTYPE, TRIAL_LANES, WINDOW_DTYPE, WINDOW_GAIN_ADD, WINDOW_GAIN_STORE, load_library, make_parameter)


def _check(where, rc):
    if rc != AADApiResult.OK:
        raise ApiError(where, rc)


def _round_up(v, a):
    return (v + a - 1) // a * a


def tensor_span(t):
    """Elements from t.data_ptr() to the end of the tensor's own storage span: 1 + sum((size - 1) * stride), 0 for an empty tensor.
    What lies behind it in the same storage belongs to somebody else as far as a run is concerned."""
    if any(int(s) == 0 for s in t.shape):
        return 0
    return 1 + sum((int(s) - 1) * int(st) for s, st in zip(t.shape, t.stride()))


def run_extent(kind, descs=None, channels=1, channel_stride=0, stream_stride=0, rows=0, frames=0):
    """Elements, counted from the pointer a run is handed, that the run may read or write, as include/aad_hip.h defines each
    call's reads and writes over the plan's table (`descs`, STREAM_DESC_DTYPE; a stream without samples or bytes touches nothing):
      "interleaved"  max(pcm_offset + num_samples * C)                          int16 frames of EncodePlan / DecodePlan runs
      "planar"       max(pcm_offset + (C - 1) * channel_stride + num_samples)   input rows of the planar and window reconstruct plans
      "images"       max(data_offset + data_size)                               bytes of every plan's images
      "planar_out"   (N - 1) * stream_stride + (C - 1) * channel_stride + the longest num_samples
      "window_rows"  rows * C * frames                                          [N, C, T] of the window plans
      "stats"        rows * C * 4                                               int64 [N, C, 4]
      "state"        rows * C * 10                                              int32 [N * C, 10]
    Python integers throughout: an offset past 2^63 does not wrap."""
    c = int(channels)
    if kind == "window_rows":
        return int(rows) * c * int(frames)
    if kind == "stats":
        return int(rows) * c * 4
    if kind == "state":
        return int(rows) * c * 10
    n = [int(v) for v in descs["num_samples"]]
    if kind == "interleaved":
        return max([int(o) + v * c for o, v in zip(descs["pcm_offset"], n) if v], default=0)
    if kind == "planar":
        return max([int(o) + (c - 1) * int(channel_stride) + v for o, v in zip(descs["pcm_offset"], n) if v], default=0)
    if kind == "images":
        return max([int(o) + int(s) for o, s in zip(descs["data_offset"], descs["data_size"]) if int(s)], default=0)
    if kind == "planar_out":
        return (len(n) - 1) * int(stream_stride) + (c - 1) * int(channel_stride) + max(n) if n and max(n) else 0
    raise ValueError("unknown extent kind %r" % (kind,))


class Engine:
    """One HIP context (device + stream).  By default it rides on torch's current stream so that
    torch.cuda.Event timing and tensor lifetimes line up with the kernels."""

    def __init__(self, device=0, stream="torch", lib=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("aad_amd.Engine needs a HIP device (torch.cuda.is_available() is False)")
        self.torch = torch
        self.lib = lib or load_library()
        self.device = int(device)
        torch.cuda.set_device(self.device)
        self.tensor_device = torch.device("cuda", self.device)  # where every tensor argument must live (tensor)
        # The C context launches on an explicit stream.  Use torch's current stream when it is a
        # real one; the legacy null stream cannot be named through a pointer, so in that case the
        # engine owns a torch side stream and orders it against the caller's stream around every
        # run (see _enter/_exit).  `with torch.cuda.stream(engine.stream):` avoids even that.
        if stream == "torch":
            cur = torch.cuda.current_stream(self.device)
            self.stream = cur if cur.cuda_stream != 0 else torch.cuda.Stream(self.device)
        elif stream is None:
            self.stream = torch.cuda.Stream(self.device)
        else:
            self.stream = stream  # a torch.cuda.Stream
        self._ctx = C.c_void_p()
        _check("AADHip_ContextCreate",
               self.lib.AADHip_ContextCreate(self.device, self.stream.cuda_stream, C.byref(self._ctx)))

    def _enter(self):
        cur = self.torch.cuda.current_stream(self.device)
        if cur.cuda_stream != self.stream.cuda_stream:
            self.stream.wait_stream(cur)
        return cur

    def _exit(self, cur):
        if cur.cuda_stream != self.stream.cuda_stream:
            cur.wait_stream(self.stream)

    # ---- the one check of a tensor argument ---------------------------------------------------
    def tensor(self, name, t, dtypes, extent=0, dims=None, shape=None, rows_in_place=False, contiguous=False, memo=None):
        """The C ABI takes raw pointers, so what a tensor is gets checked here, before any library call: dtype (one or several),
        device (this engine's), rank (`dims`) or shape (None: any size), strides - rows_in_place: stride(-1) == 1, the rows are read
        or written where they lie; contiguous: the C call has no stride to give - and extent: the elements the run touches from
        data_ptr() (run_extent) against the tensor's own span (tensor_span).  ValueError names the argument, the need and the given.
        memo: a plan's dict.  The verdict depends on the tensor's shape, strides, dtype and device alone (the rules of one argument
        of one plan never change), so a run that is handed the same layout again - a training loop's every step - skips the rest."""
        torch = self.torch
        if not torch.is_tensor(t):
            raise ValueError("%s: a torch tensor is needed, got %s" % (name, type(t).__name__))
        if memo is not None:
            key = (t.shape, t.stride(), t.dtype, t.device)
            if memo.get(name) == key:
                return t
        dtypes = tuple(dtypes) if isinstance(dtypes, (tuple, list)) else (dtypes,)
        if t.dtype not in dtypes:
            raise ValueError("%s: dtype %s is needed, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
        if t.device != self.tensor_device:
            raise ValueError("%s: a tensor on the engine's device %s is needed, got one on %s" % (name, self.tensor_device, t.device))
        if dims is not None and t.dim() != dims:
            raise ValueError("%s: %d dimensions are needed, got shape %s" % (name, dims, tuple(t.shape)))
        if shape is not None and (t.dim() != len(shape) or any(w is not None and int(w) != int(g) for w, g in zip(shape, t.shape))):
            raise ValueError("%s: shape [%s] is needed, got %s" % (name, ", ".join("*" if w is None else str(int(w)) for w in shape),
                                                                 tuple(t.shape)))
        if rows_in_place and t.dim() and int(t.shape[-1]) > 1 and t.stride(-1) != 1:
            raise ValueError("%s: stride(-1) == 1 is needed (its rows are read or written where they lie); got strides %s - pass "
                             "%s.contiguous() if a copy is intended" % (name, tuple(t.stride()), name))
        if contiguous and not t.is_contiguous():
            raise ValueError("%s: a contiguous tensor is needed (the C call takes no strides for it); got shape %s with strides %s - "
                             "pass %s.contiguous() if a copy is intended" % (name, tuple(t.shape), tuple(t.stride()), name))
        if tensor_span(t) < extent:
            raise ValueError("%s: the run touches %d elements from data_ptr(), the tensor spans %d (shape %s, strides %s)"
                             % (name, extent, tensor_span(t), tuple(t.shape), tuple(t.stride())))
        if memo is not None:
            memo[name] = key
        return t

    def state_tensor(self, state, streams, channels, memo=None):
        """state: None, or the contiguous int32 [streams * channels, 10] table of AADHipLaneState records a run reads and writes"""
        if state is not None:
            lanes = int(streams) * int(channels)
            self.tensor("state", state, self.torch.int32, run_extent("state", rows=streams, channels=channels), shape=(lanes, 10),
                        contiguous=True, memo=memo)
        return state

    def planar_input(self, what, name, x, param, num_samples, shortest=1):
        """x: the int16 or float32 [N, C, T] view a planar entry point reads in place; num_samples: per-row lengths in
        [shortest, T], default T -> (N, C, T, lengths)"""
        torch = self.torch
        self.tensor(name, x, (torch.int16, torch.float32), dims=3, rows_in_place=True)
        n, ch, t = (int(v) for v in x.shape)
        if param is not None and ch != param.num_channels:
            raise ValueError("%s: %s has %d channels, the parameter %d" % (what, name, ch, param.num_channels))
        lengths = np.full(n, t, dtype=np.int64) if num_samples is None else np.asarray(num_samples, dtype=np.int64).reshape(-1)
        if len(lengths) != n or (n and (lengths.min() < shortest or lengths.max() > t)):
            raise ValueError("num_samples: %d lengths in [%d, %d]" % (n, shortest, t))
        if ch > 1 and n and x.stride(1) < int(lengths.max()):
            raise ValueError("%s: %s has channel stride %d (stride(1)) below its longest row of %d samples - the channels' rows would "
                             "overlap; pass %s.contiguous() if a copy is intended" % (what, name, x.stride(1), int(lengths.max()), name))
        return n, ch, t, lengths

    def window_table(self, windows, ordered, name="windows", rows=None):
        """windows: int64 [N, 2] of (stream, first_frame) on the device -> the contiguous table the C call takes.
        name="spans", rows=N: the span table of a run with spans, int64 [N, 2] of (num_frames, out_frame), by the same rules.
        A non-contiguous one is copied.  The copy is a temporary that goes back to torch's caching allocator when the run
        returns, while the kernel may not have read it yet.  With ordered=True that is safe: the allocator hands a block out again
        to work on the stream it was allocated on, torch's current stream, and _exit has made that stream wait for the engine's, so
        whatever reuses the block is queued behind the kernel.  With ordered=False nothing orders the two streams and the
        kernel could read a table that has been handed out again: refused, the caller keeps a contiguous table alive."""
        self.tensor(name, windows, self.torch.int64, shape=(rows, 2))
        if not windows.is_contiguous():
            if not ordered:
                raise ValueError("%s: a contiguous tensor is needed with ordered=False (a temporary copy could be freed and "
                                 "reused while the kernel still reads it); got strides %s - keep %s.contiguous() alive until "
                                 "the run is done" % (name, tuple(windows.stride()), name))
            windows = windows.contiguous()
        return windows

    def interleaved_input(self, what, pcm, param):
        """pcm: the contiguous int16 [streams, samples, channels] tensor of the uniform entry points -> (streams, samples, channels).
        The interleaved C calls take one offset per stream and no stride, so a view cannot be read in place."""
        self.tensor("pcm", pcm, self.torch.int16, dims=3, contiguous=True)
        streams, samples, ch = (int(v) for v in pcm.shape)
        if ch != param.num_channels:
            raise ValueError("%s: pcm has %d channels, the parameter %d" % (what, ch, param.num_channels))
        return streams, samples, ch

    def image_rows(self, name, data, image_sizes):
        """data: uint8 [streams, pitch] whose rows start with an image each, read in place -> the per-row image sizes (uint64)"""
        self.tensor(name, data, self.torch.uint8, dims=2, rows_in_place=True)
        s, width = int(data.shape[0]), int(data.shape[1])
        if s == 0:
            raise ValueError("%s: at least one image is needed (the format comes from the headers), got shape %s" % (name, tuple(data.shape)))
        sizes = np.broadcast_to(np.asarray(image_sizes, dtype=np.uint64).reshape(-1), (s,))
        if int(sizes.max()) > width:
            raise ValueError("%s: an image of %d bytes is needed in every row, the rows have %d (shape %s)"
                             % (name, int(sizes.max()), width, tuple(data.shape)))
        return sizes

    def close(self):
        if self._ctx:
            self.lib.AADHip_ContextDestroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def signal_next(self, stop, start=None):
        """stop / start: HipEvent (or None) - recorded when the work of the NEXT plan run on this engine is done / starts,
        carried by the run's own kernel dispatch instead of packets around it (AADHip_ContextSignalNextRun)"""
        _check("AADHip_ContextSignalNextRun",
               self.lib.AADHip_ContextSignalNextRun(self._ctx, start.handle if start is not None else None,
                                                    stop.handle if stop is not None else None))

    def last_error(self):
        return (self.lib.AADHip_ContextLastError(self._ctx) or b"").decode()

    def set_mapping(self, mapping="auto", trial_lanes=None):
        """Force a lane mapping ("auto", "dense", "quad", "quad-fused") and, optionally, the trial
        search's lane layout ("dual", "single") for every later run of this context
        (AADHip_ContextSetOption; the environment is only read when the context is created)."""
        _check("AADHip_ContextSetOption",
               self.lib.AADHip_ContextSetOption(self._ctx, OPTION_LANE_MAPPING, LANE_MAPPINGS[mapping or "auto"]))
        if trial_lanes is not None:
            _check("AADHip_ContextSetOption",
                   self.lib.AADHip_ContextSetOption(self._ctx, OPTION_TRIAL_LANES, TRIAL_LANES[trial_lanes]))

    def set_staging_threads(self, threads=0):
        """Threads that copy between caller buffers and the pinned staging blocks in the host-memory
        entry points: 0 = by core count, 1 = the calling thread alone, up to 8."""
        _check("AADHip_ContextSetOption",
               self.lib.AADHip_ContextSetOption(self._ctx, OPTION_STAGING_THREADS, int(threads)))

    def set_tile_kbytes(self, kbytes=0):
        """Tile budget (KiB) of the host-memory entry points; 0 = built in.  Results do not depend on it."""
        _check("AADHip_ContextSetOption",
               self.lib.AADHip_ContextSetOption(self._ctx, OPTION_TILE_KBYTES, int(kbytes)))

    def set_compare_order(self, sequential=False):
        """fp64 summation order behind the reconstruction modes' statistics: False = tree on the device with the
        reference's order taken only next to a rounding boundary of the printed line, True = always the reference's order
        (bit-identical doubles; AAD_HIP_OPTION_COMPARE_ORDER)"""
        _check("AADHip_ContextSetOption",
               self.lib.AADHip_ContextSetOption(self._ctx, OPTION_COMPARE_ORDER, 1 if sequential else 0))

    def set_simd_role(self, simd=None):
        """The SIMD (0..3) of a CU that runs the one busy wave of this context's lane-starved launches (the quad encoder, the
        split decoder's recurrence wave), None = off: today's launches.  Contexts whose kernels run side by side take different
        SIMDs (EncodeDecodePipeline does); the bytes never depend on it (AAD_HIP_OPTION_SIMD_ROLE)."""
        _check("AADHip_ContextSetOption",
               self.lib.AADHip_ContextSetOption(self._ctx, OPTION_SIMD_ROLE, SIMD_ROLE_OFF if simd is None else int(simd)))

    def synchronize(self):
        _check("AADHip_ContextSynchronize", self.lib.AADHip_ContextSynchronize(self._ctx))

    def encoded_size(self, param, num_samples):
        return int(self.lib.AADHip_CalculateEncodedSize(C.byref(param), num_samples))

    # ---- plans ---------------------------------------------------------------------------
    def encode_plan(self, param, descs, segment_blocks=None, warmup_blocks=0):
        """segment_blocks: None for the reference encoder's bytes, else a segmented plan
        (AADHip_SegmentedEncodePlanCreate): chains of segment_blocks kept blocks, each after warmup_blocks
        discarded ones - a valid stream, not the reference encoder's bytes (include/aad_hip.h)."""
        descs = np.ascontiguousarray(descs, dtype=STREAM_DESC_DTYPE)
        plan = C.c_void_p()
        if segment_blocks is None:
            _check("AADHip_EncodePlanCreate",
                   self.lib.AADHip_EncodePlanCreate(self._ctx, C.byref(param), len(descs), descs.ctypes.data, C.byref(plan)))
        else:
            seg = AADHipSegmentation(int(segment_blocks), int(warmup_blocks))
            _check("AADHip_SegmentedEncodePlanCreate",
                   self.lib.AADHip_SegmentedEncodePlanCreate(self._ctx, C.byref(param), C.byref(seg), len(descs),
                                                             descs.ctypes.data, C.byref(plan)))
        p = EncodePlan(self, plan, param, descs)
        p.segmented = segment_blocks is not None
        return p

    def planar_encode_plan(self, param, descs, channel_stride, dtype, segment_blocks=None, warmup_blocks=0):
        """A plan over planar input (AADHip_PlanarEncodePlanCreate): stream i's channel c is the row of num_samples elements at
        pcm_offset + c * channel_stride of a torch.int16 or torch.float32 buffer (float32: sample * 32768, rounded to even and
        clamped, NaN as 0).  The bytes are encode_plan's on the interleaved int16 of those samples; segment_blocks /
        warmup_blocks as there.  PlanarEncodePlan.run encodes."""
        torch = self.torch
        if dtype not in (torch.int16, torch.float32):
            raise ValueError("planar encode reads torch.int16 or torch.float32 rows, not %s" % dtype)
        descs = np.ascontiguousarray(descs, dtype=STREAM_DESC_DTYPE)
        layout = AADHipPlanarLayout(SAMPLE_FLOAT32 if dtype == torch.float32 else SAMPLE_INT16, 0, int(channel_stride))
        seg = AADHipSegmentation(int(segment_blocks), int(warmup_blocks)) if segment_blocks is not None else None
        plan = C.c_void_p()
        _check("AADHip_PlanarEncodePlanCreate",
               self.lib.AADHip_PlanarEncodePlanCreate(self._ctx, C.byref(param), C.byref(layout), C.byref(seg) if seg is not None else None,
                                                      len(descs), descs.ctypes.data, C.byref(plan)))
        p = PlanarEncodePlan(self, plan, param, descs, dtype, int(channel_stride))
        p.segmented = segment_blocks is not None
        return p

    def planar_reconstruct_plan(self, param, descs, channel_stride, dtype, out_dtype, out_stream_stride, out_channel_stride,
                                segment_blocks=None, warmup_blocks=0):
        """A planar encode plan that also writes the decoded rows (AADHip_PlanarReconstructPlanCreate): input as planar_encode_plan,
        output stream i's channel c at i * out_stream_stride + c * out_channel_stride elements of a torch.int16 or torch.float32
        tensor (float32: decoded sample / 32768).  PlanarReconstructPlan.run encodes and reconstructs in one kernel."""
        torch = self.torch
        if dtype not in (torch.int16, torch.float32) or out_dtype not in (torch.int16, torch.float32):
            raise ValueError("planar reconstruct reads and writes torch.int16 or torch.float32 rows, not %s -> %s" % (dtype, out_dtype))
        descs = np.ascontiguousarray(descs, dtype=STREAM_DESC_DTYPE)
        layout = AADHipPlanarLayout(SAMPLE_FLOAT32 if dtype == torch.float32 else SAMPLE_INT16, 0, int(channel_stride))
        output = AADHipPlanarOutput(SAMPLE_FLOAT32 if out_dtype == torch.float32 else SAMPLE_INT16, 0, int(out_stream_stride),
                                    int(out_channel_stride))
        seg = AADHipSegmentation(int(segment_blocks), int(warmup_blocks)) if segment_blocks is not None else None
        plan = C.c_void_p()
        _check("AADHip_PlanarReconstructPlanCreate",
               self.lib.AADHip_PlanarReconstructPlanCreate(self._ctx, C.byref(param), C.byref(layout), C.byref(output),
                                                           C.byref(seg) if seg is not None else None, len(descs), descs.ctypes.data,
                                                           C.byref(plan)))
        p = PlanarReconstructPlan(self, plan, param, descs, dtype, out_dtype, int(channel_stride), int(out_stream_stride),
                                  int(out_channel_stride))
        p.segmented = segment_blocks is not None
        return p

    def window_reconstruct_plan(self, param, source_table, channel_stride, dtype, segment_blocks=None, warmup_blocks=0):
        """A plan over a PCM corpus on the device (AADHip_WindowReconstructPlanCreate): source stream s is num_samples frames whose
        channel c is the row at pcm_offset + c * channel_stride elements of a torch.int16 or torch.float32 buffer (the other fields
        of source_table are ignored).  WindowReconstructPlan.run puts crops of it, named by a window table on the device, through
        the codec: decoded rows, exact error statistics, images, or any subset.  segment_blocks / warmup_blocks as encode_plan."""
        torch = self.torch
        if dtype not in (torch.int16, torch.float32):
            raise ValueError("window reconstruct reads torch.int16 or torch.float32 rows, not %s" % dtype)
        source_table = np.ascontiguousarray(source_table, dtype=STREAM_DESC_DTYPE)
        layout = AADHipPlanarLayout(SAMPLE_FLOAT32 if dtype == torch.float32 else SAMPLE_INT16, 0, int(channel_stride))
        seg = AADHipSegmentation(int(segment_blocks), int(warmup_blocks)) if segment_blocks is not None else None
        plan = C.c_void_p()
        _check("AADHip_WindowReconstructPlanCreate",
               self.lib.AADHip_WindowReconstructPlanCreate(self._ctx, C.byref(param), C.byref(layout),
                                                           C.byref(seg) if seg is not None else None, len(source_table),
                                                           source_table.ctypes.data, C.byref(plan)))
        p = WindowReconstructPlan(self, plan, param, source_table, dtype, int(channel_stride))
        p.segmented = segment_blocks is not None
        return p

    def decode_plan(self, header, descs, has_file_header=True):
        descs = np.ascontiguousarray(descs, dtype=STREAM_DESC_DTYPE)
        plan = C.c_void_p()
        _check("AADHip_DecodePlanCreate",
               self.lib.AADHip_DecodePlanCreate(self._ctx, C.byref(header), 1 if has_file_header else 0, len(descs),
                                                descs.ctypes.data, C.byref(plan)))
        return DecodePlan(self, plan, header, descs)

    def window_decode_plan(self, header, descs, has_file_header=True):
        """A stream table for window decodes (AADHip_WindowDecodePlanCreate; pcm_offset is ignored): WindowDecodePlan.run
        decodes crops [first_frame, first_frame + frames) of any streams of it into planar [N, C, T] rows."""
        descs = np.ascontiguousarray(descs, dtype=STREAM_DESC_DTYPE)
        plan = C.c_void_p()
        _check("AADHip_WindowDecodePlanCreate",
               self.lib.AADHip_WindowDecodePlanCreate(self._ctx, C.byref(header), 1 if has_file_header else 0, len(descs),
                                                      descs.ctypes.data, C.byref(plan)))
        return WindowDecodePlan(self, plan, header, descs)

    def mixed_window_decode_plan(self, headers, descs, has_file_header=True, num_channels=None):
        """A stream table for window decodes over streams that do not share a format (AADHip_MixedWindowDecodePlanCreate):
        headers[i] is stream i's AADHeaderInfo - bits, block size, samples per block and mid/side may differ from stream to stream,
        the channel count may not (num_channels: default headers[0]'s; needed only for an empty table).  The WindowDecodePlan it
        returns runs one kernel per (bits, mid/side) pair among the headers."""
        descs = np.ascontiguousarray(descs, dtype=STREAM_DESC_DTYPE)
        headers = list(headers)
        if len(headers) != len(descs):
            raise ValueError("%d headers for %d streams" % (len(headers), len(descs)))
        if num_channels is None:
            if not headers:
                raise ValueError("an empty table needs num_channels")
            num_channels = headers[0].num_channels
        formats = (AADHeaderInfo * max(len(headers), 1))(*headers)
        plan = C.c_void_p()
        _check("AADHip_MixedWindowDecodePlanCreate",
               self.lib.AADHip_MixedWindowDecodePlanCreate(self._ctx, int(num_channels), 1 if has_file_header else 0, len(descs),
                                                           descs.ctypes.data, C.addressof(formats), C.byref(plan)))
        p = WindowDecodePlan(self, plan, AADHeaderInfo(num_channels=int(num_channels)), descs)
        p.headers = headers
        return p

    def channel_mix_window_decode_plan(self, headers, descs, out_channels, has_file_header=True):
        """A stream table for window decodes over mono and stereo streams into rows of one channel count
        (AADHip_ChannelMixWindowDecodePlanCreate): headers[i] is stream i's AADHeaderInfo - the channel count (1 or 2), bits, block
        size, samples per block and mid/side may differ from stream to stream.  out_channels = 2 writes a mono stream into both
        rows; out_channels = 1 writes a stereo stream's mean, (L + R) >> 1 as int16 and (L + R) / 65536 as float32.  The
        WindowDecodePlan it returns runs one kernel per (channels, bits, mid/side) among the headers."""
        descs = np.ascontiguousarray(descs, dtype=STREAM_DESC_DTYPE)
        headers = list(headers)
        if len(headers) != len(descs):
            raise ValueError("%d headers for %d streams" % (len(headers), len(descs)))
        formats = (AADHeaderInfo * max(len(headers), 1))(*headers)
        plan = C.c_void_p()
        _check("AADHip_ChannelMixWindowDecodePlanCreate",
               self.lib.AADHip_ChannelMixWindowDecodePlanCreate(self._ctx, int(out_channels), 1 if has_file_header else 0, len(descs),
                                                                descs.ctypes.data, C.addressof(formats), C.byref(plan)))
        p = WindowDecodePlan(self, plan, AADHeaderInfo(num_channels=int(out_channels)), descs)
        p.headers = headers
        return p

    # ---- uniform batches (every stream the same length) -----------------------------------
    def uniform_encode_plan(self, param, num_streams, num_samples, segment_blocks=None, warmup_blocks=0):
        """Stream table for a [streams, samples, channels] int16 tensor and a [streams, stride]
        uint8 output; stride = encoded size rounded up to 64 bytes (images on 64-byte boundaries let the
        dense stereo encoder store whole granules - aad_encode.hip.h run_block)."""
        size = self.encoded_size(param, num_samples)
        if size == 0:
            raise ApiError("AADHip_CalculateEncodedSize", AADApiResult.INVALID_FORMAT)
        stride = _round_up(size, 64)
        d = np.zeros(num_streams, dtype=STREAM_DESC_DTYPE)
        i = np.arange(num_streams, dtype=np.uint64)
        d["pcm_offset"] = i * np.uint64(num_samples * param.num_channels)
        d["data_offset"] = i * np.uint64(stride)
        d["data_size"] = stride
        d["num_samples"] = num_samples
        plan = self.encode_plan(param, d, segment_blocks, warmup_blocks)
        plan.image_size, plan.stride = size, stride
        return plan

    def uniform_decode_plan(self, header, num_streams, stride, image_size):
        d = np.zeros(num_streams, dtype=STREAM_DESC_DTYPE)
        i = np.arange(num_streams, dtype=np.uint64)
        d["pcm_offset"] = i * np.uint64(header.num_samples * header.num_channels)
        d["data_offset"] = i * np.uint64(stride)
        d["data_size"] = image_size
        d["num_samples"] = header.num_samples
        return self.decode_plan(header, d, True)

    def encode_uniform(self, pcm, param, state=None, segment_blocks=None, warmup_blocks=0):
        """pcm: int16 cuda tensor [streams, samples, channels] -> uint8 tensor [streams, stride]
        (each row starts with a complete .aad image of plan.image_size bytes).  segment_blocks / warmup_blocks:
        a segmented encode (see encode_plan), which takes no state."""
        torch = self.torch
        if state is not None and segment_blocks is not None:
            raise ValueError("a segmented encode starts from fresh encoders: state and segment_blocks exclude each other")
        streams, samples, ch = self.interleaved_input("encode_uniform", pcm, param)
        self.state_tensor(state, streams, ch)
        plan = self.uniform_encode_plan(param, streams, samples, segment_blocks, warmup_blocks)
        out = torch.zeros((streams, plan.stride), dtype=torch.uint8, device=pcm.device)
        plan.run(pcm, out, state)
        return out, plan.image_size

    def encode_planar(self, x, param, num_samples=None, state=None, segment_blocks=None, warmup_blocks=0):
        """x: int16 or float32 cuda tensor [N, C, T] - a view is fine as long as x.stride(-1) == 1 - -> (uint8 tensor [N, stride],
        image_sizes): row i starts with the .aad image of x[i, :, :num_samples[i]] (num_samples: per-row lengths <= T, default T),
        image_sizes[i] bytes long; rows lie on 64-byte boundaries as in encode_uniform.  float32 samples are read as
        sample * 32768 (rounded to even, clamped, NaN as 0); the rows are encoded where they are, with no copy or conversion pass."""
        torch = self.torch
        if state is not None and segment_blocks is not None:
            raise ValueError("a segmented encode starts from fresh encoders: state and segment_blocks exclude each other")
        n, ch, t, lengths = self.planar_input("encode_planar", "x", x, param, num_samples)
        self.state_tensor(state, n, ch)
        sizes = np.array([self.encoded_size(param, int(v)) for v in lengths], dtype=np.uint64)
        if n and sizes.min() == 0:
            raise ApiError("AADHip_CalculateEncodedSize", AADApiResult.INVALID_FORMAT)
        stride = _round_up(int(sizes.max()), 64) if n else 64
        d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
        d["pcm_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(x.stride(0))
        d["data_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        d["data_size"] = stride
        d["num_samples"] = lengths
        out = torch.zeros((n, stride), dtype=torch.uint8, device=x.device)
        plan = self.planar_encode_plan(param, d, x.stride(1), x.dtype, segment_blocks, warmup_blocks)
        try:
            plan.run(x, out, state)
        finally:
            plan.close()  # synchronises the context's stream first
        return out, [int(v) for v in sizes]

    def encode_planar_mixed(self, x, make_param, bits, num_samples=None):
        """encode_planar with a parameter per row: bits is an int sequence or tensor [N] of 2, 3 or 4 (what least_bits returns, once
        its zeros are decided), make_param(b) the AADEncodeParameter of the rows with bits b -> (uint8 tensor [N, stride],
        image_sizes).  Row i starts with the image encode_planar(x[i:i + 1], make_param(bits[i])) writes, byte for byte; the rows
        lie on 64-byte boundaries.  One planar encode plan per value of bits that occurs, its descriptor table naming that value's
        rows where they are: no gather of x."""
        torch = self.torch
        n, ch, t, lengths = self.planar_input("encode_planar_mixed", "x", x, None, num_samples)  # the channels: per parameter, below
        bits = (bits.detach().cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)).astype(np.int64).reshape(-1)
        if len(bits) != n or not np.isin(bits, (2, 3, 4)).all():
            raise ValueError("bits: %d values of 2, 3 or 4" % n)
        params = {int(b): make_param(int(b)) for b in np.unique(bits)}
        for b, param in params.items():
            if param.num_channels != ch or param.bits_per_sample != b:
                raise ValueError("make_param(%d): %d channels and %d bits for rows of %d channels"
                                 % (b, param.num_channels, param.bits_per_sample, ch))
        sizes = np.array([self.encoded_size(params[int(b)], int(v)) for b, v in zip(bits, lengths)], dtype=np.uint64)
        if n and sizes.min() == 0:
            raise ApiError("AADHip_CalculateEncodedSize", AADApiResult.INVALID_FORMAT)
        stride = _round_up(int(sizes.max()), 64) if n else 64
        out = torch.zeros((n, stride), dtype=torch.uint8, device=x.device)
        for b, param in params.items():
            rows = np.flatnonzero(bits == b)
            d = np.zeros(len(rows), dtype=STREAM_DESC_DTYPE)
            d["pcm_offset"] = rows.astype(np.uint64) * np.uint64(x.stride(0))
            d["data_offset"] = rows.astype(np.uint64) * np.uint64(stride)
            d["data_size"] = stride
            d["num_samples"] = lengths[rows]
            plan = self.planar_encode_plan(param, d, x.stride(1), x.dtype)
            try:
                plan.run(x, out)
            finally:
                plan.close()  # synchronises the context's stream first
        return out, [int(v) for v in sizes]

    def reconstruct_planar(self, x, param, num_samples=None, dtype=None, state=None, segment_blocks=None, warmup_blocks=0,
                           return_images=False, return_stats=False):
        """x: int16 or float32 cuda tensor [N, C, T] (a view with x.stride(-1) == 1 is fine) -> a new contiguous [N, C, T] tensor of
        `dtype` (default x.dtype): x after the codec - row i is the decode of encode_planar's image of x[i, :, :num_samples[i]]
        (float32 output: decoded sample / 32768), zero past num_samples[i].  One kernel: the encoder writes the decoded rows as it
        encodes.  return_images=True: (y, images, image_sizes) with images and sizes in encode_planar's layout.
        return_stats=True appends the int64 [N, C, 4] tensor of exact per-row error statistics (sum_sq, sum_abs, max_abs, count of
        q(x) - decoded sample in int16 units; include/aad_hip.h), accumulated by the same kernel: see rmse / snr_db."""
        return self._reconstruct_planar("reconstruct_planar", x, param, num_samples, dtype, state, segment_blocks, warmup_blocks,
                                        True, return_images, return_stats)

    def codec_error(self, x, param, num_samples=None, state=None, segment_blocks=None, warmup_blocks=0):
        """The statistics of reconstruct_planar(..., return_stats=True) alone - int64 [N, C, 4] - with no rows allocated or written."""
        return self._reconstruct_planar("codec_error", x, param, num_samples, None, state, segment_blocks, warmup_blocks,
                                        False, False, True)

    def least_bits(self, x, make_param, min_snr_db, num_samples=None):
        """Per stream the fewest bits per sample (2, 3 or 4) at which every channel keeps an SNR of at least min_snr_db, 0 where
        none does: int64 cuda tensor [N].  make_param(bits) returns the AADEncodeParameter to try.  The signal power is that of
        q(x), the int16 samples the encoder sees."""
        torch = self.torch
        n, _, t = (int(v) for v in x.shape)
        lengths = torch.full((n,), t, dtype=torch.int64) if num_samples is None else torch.as_tensor(np.asarray(num_samples, dtype=np.int64))
        q = x if x.dtype == torch.int16 else torch.nan_to_num(x, nan=0.0).mul(32768.0).round().clamp(-32768, 32767)
        live = torch.arange(t, device=x.device)[None, None, :] < lengths.to(x.device)[:, None, None]
        signal = (q.to(torch.float64) ** 2 * live).sum(-1)  # squares below 2^30, fewer than 2^23 of them per partial sum: exact
        return select_least_bits([snr_db(self.codec_error(x, make_param(bits), num_samples), signal) for bits in (2, 3, 4)], min_snr_db)

    def _reconstruct_planar(self, what, x, param, num_samples, dtype, state, segment_blocks, warmup_blocks, rows, return_images,
                            return_stats):
        torch = self.torch
        if state is not None and segment_blocks is not None:
            raise ValueError("a segmented encode starts from fresh encoders: state and segment_blocks exclude each other")
        n, ch, t, lengths = self.planar_input(what, "x", x, param, num_samples)
        self.state_tensor(state, n, ch)
        dtype = x.dtype if dtype is None else dtype
        sizes = np.array([self.encoded_size(param, int(v)) for v in lengths], dtype=np.uint64)
        if n and sizes.min() == 0:
            raise ApiError("AADHip_CalculateEncodedSize", AADApiResult.INVALID_FORMAT)
        stride = _round_up(int(sizes.max()), 64) if n else 64
        d = np.zeros(n, dtype=STREAM_DESC_DTYPE)
        d["pcm_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(x.stride(0))
        d["data_offset"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        d["data_size"] = stride
        d["num_samples"] = lengths
        images = torch.zeros((n, stride), dtype=torch.uint8, device=x.device)
        y = torch.zeros((n, ch, t), dtype=dtype, device=x.device) if rows else None
        stats = torch.empty((n, ch, 4), dtype=torch.int64, device=x.device) if return_stats else None  # every record is written
        plan = self.planar_reconstruct_plan(param, d, x.stride(1), x.dtype, dtype, ch * t, t, segment_blocks, warmup_blocks)
        try:
            plan.run(x, images, y, state, stats=stats)
        finally:
            plan.close()  # synchronises the context's stream first
        result = ([y] if rows else []) + ([images, [int(v) for v in sizes]] if return_images else []) + ([stats] if return_stats else [])
        return result[0] if len(result) == 1 else tuple(result)

    def reconstruct_windows(self, corpus, windows, frames, param, dtype=None, return_images=False, return_stats=False,
                            num_samples=None, segment_blocks=None, warmup_blocks=0):
        """corpus: int16 or float32 cuda tensor [S, C, T_total] (a view with corpus.stride(-1) == 1 is fine); windows: int64 cuda
        tensor [N, 2] of (stream, first_frame), never read on the host -> a new [N, C, frames] tensor of `dtype` (default
        corpus.dtype): crop w = corpus[stream, :, first_frame:first_frame + frames] after the codec, as reconstruct_planar gives it
        for the gathered crops, zero where the crop runs past its stream (num_samples: per-stream lengths <= T_total, default
        T_total) and all zero for a stream index past S.  No gather and no copy of the batch: a kernel writes the encoders' tables
        from the windows where they are.  The call makes a plan and closes it, which synchronises the engine's stream, as
        reconstruct_planar does; a training loop keeps a window_reconstruct_plan and calls its run, which is asynchronous.  return_images=True: (y, images, stride) with window w's image at the
        start of images[w] (its length follows from bytes 14..17, or from the statistics' count); return_stats=True appends the
        int64 [N, C, 4] statistics of reconstruct_planar."""
        return self._reconstruct_windows("reconstruct_windows", corpus, windows, frames, param, dtype, num_samples, segment_blocks,
                                         warmup_blocks, True, return_images, return_stats)

    def codec_error_windows(self, corpus, windows, frames, param, num_samples=None, segment_blocks=None, warmup_blocks=0):
        """The statistics of reconstruct_windows(..., return_stats=True) alone - int64 [N, C, 4] - with no rows or images allocated."""
        return self._reconstruct_windows("codec_error_windows", corpus, windows, frames, param, None, num_samples, segment_blocks,
                                         warmup_blocks, False, False, True)

    def _reconstruct_windows(self, what, corpus, windows, frames, param, dtype, num_samples, segment_blocks, warmup_blocks, rows,
                             return_images, return_stats):
        torch = self.torch
        s, ch, t, lengths = self.planar_input(what, "corpus", corpus, param, num_samples, shortest=0)
        self.tensor("windows", windows, torch.int64, shape=(None, 2))
        d = np.zeros(s, dtype=STREAM_DESC_DTYPE)
        d["pcm_offset"] = np.arange(s, dtype=np.uint64) * np.uint64(corpus.stride(0))
        d["num_samples"] = lengths
        plan = self.window_reconstruct_plan(param, d, corpus.stride(1), corpus.dtype, segment_blocks, warmup_blocks)
        try:
            n = int(windows.shape[0])
            stride = _round_up(self.encoded_size(param, int(frames)), 64)
            images = torch.empty((n, stride), dtype=torch.uint8, device=corpus.device) if return_images else None
            stats = torch.empty((n, ch, 4), dtype=torch.int64, device=corpus.device) if return_stats else None
            y = plan.run(corpus, windows, frames, dtype=corpus.dtype if dtype is None else dtype, data=images, stats=stats) if rows \
                else plan.run(corpus, windows, frames, out=False, data=images, stats=stats)
        finally:
            plan.close()  # synchronises the context's stream first
        result = ([y] if rows else []) + ([images, stride] if return_images else []) + ([stats] if return_stats else [])
        return result[0] if len(result) == 1 else tuple(result)

    def decode_uniform(self, data, image_size):
        """data: uint8 cuda tensor [streams, pitch] of same-format images, image_size <= pitch bytes each; a view is fine as long as
        data.stride(1) == 1: row i is read where it lies, at i * data.stride(0) -> int16 [streams, samples, channels]"""
        torch = self.torch
        self.image_rows("data", data, image_size)
        head = bytes(data[0, :31].cpu().numpy())
        header = parse_header(head)
        plan = self.uniform_decode_plan(header, data.shape[0], data.stride(0), image_size)  # the row pitch: the view's, not its width
        pcm = torch.zeros((data.shape[0], header.num_samples, header.num_channels), dtype=torch.int16, device=data.device)
        plan.run(data, pcm)
        return pcm, header

    def uniform_window_decode_plan(self, header, num_streams, stride, image_size):
        d = np.zeros(num_streams, dtype=STREAM_DESC_DTYPE)
        d["data_offset"] = np.arange(num_streams, dtype=np.uint64) * np.uint64(stride)
        d["data_size"] = image_size
        d["num_samples"] = header.num_samples
        return self.window_decode_plan(header, d, True)

    def decode_windows(self, data, image_size, windows, frames, dtype=None, return_stats=False, out=None, gain=None,
                       accumulate=False, spans=None):
        """data: uint8 cuda tensor [streams, pitch] of same-format images (encode_uniform's output, or a view of it with
        data.stride(1) == 1: row i is read where it lies, at i * data.stride(0)); windows: int64 cuda tensor
        [N, 2] of (stream, first_frame) -> [N, channels, frames] tensor of `dtype` (torch.float32 = sample / 32768, torch.int16, or
        torch.float16 / torch.bfloat16 = the float32 row rounded to nearest even).
        The header is read once, from the first image; the windows are never read on the host.
        return_stats: -> (rows, int64 [N, channels, 4] level statistics of the rows), see WindowDecodePlan.run.
        gain / accumulate / out: float rows scaled by a float32 [N] gain per window, stored or added into `out`, see there.
        spans: int64 cuda tensor [N, 2] of (num_frames, out_frame) - each crop clipped to and placed inside its row, see there."""
        self.image_rows("data", data, image_size)
        head = bytes(data[0, :31].cpu().numpy())
        header = parse_header(head)
        plan = self.uniform_window_decode_plan(header, data.shape[0], data.stride(0), image_size)  # the view's row pitch
        try:
            return plan.run(data, windows, frames, dtype, out=out, stats=True if return_stats else None, gain=gain,
                            accumulate=accumulate, spans=spans)
        finally:
            plan.close()  # synchronises the context's stream first

    def decode_windows_mixed(self, data, image_sizes, windows, frames, dtype=None, channels=None, return_stats=False, out=None,
                             gain=None, accumulate=False, spans=None):
        """decode_windows over images that do not share a format (encode_planar_mixed's output): data is a uint8 cuda tensor
        [streams, stride], row i starting with an image of image_sizes[i] bytes (an int: the same for all).  The 31-byte headers of
        all the images come to the host in one copy and are parsed one by one (the channel counts must agree); the windows are
        never read on the host.  channels = 1 or 2: mono and stereo images may share the tensor and the result has that many rows
        per window (channel_mix_window_decode_plan).  return_stats: -> (rows, int64 [N, channels, 4] level statistics).
        gain / accumulate / out: float rows scaled by a float32 [N] gain per window, stored or added into `out`;
        spans: int64 cuda tensor [N, 2] of (num_frames, out_frame), each crop clipped to and placed inside its row
        (WindowDecodePlan.run)."""
        plan = self._corpus_window_plan(data, image_sizes, channels)
        try:
            return plan.run(data, windows, frames, dtype, out=out, stats=True if return_stats else None, gain=gain,
                            accumulate=accumulate, spans=spans)
        finally:
            plan.close()  # synchronises the context's stream first

    def mix_windows(self, signal, noise, frames, snr_db, dtype=None, channels=None, noise_spans=None):
        """A noisy batch at a chosen SNR without a temporary batch or an elementwise pass.  signal, noise: each
        (data, image_sizes, windows) as for decode_windows_mixed, the same number of windows; snr_db: a number or a tensor [N].
        Two statistics-only runs give the levels, snr_gains the noise gains on the device, then one run STORES the signal rows
        and one ADDS gain * noise into them -> (rows [N, channels, frames] of `dtype`, float32 [N] noise gains).  Per element
        fl32(signal_float32 rounded to dtype, widened + fl32(gain * noise_float32)) rounded once to dtype.
        noise_spans: int64 cuda tensor [N, 2] of (num_frames, out_frame) - the noise of window w is an event of num_frames frames
        added at element out_frame of the signal's row (WindowDecodePlan.run with spans).  The noise levels then come from a
        statistics-only run over the spans, and the SNR is the signal's power over ITS counted frames - the whole row, not the
        part under the event - against the noise's power over the event's own counted frames: the level of the event while it
        sounds, not averaged over the row."""
        torch = self.torch
        dtype = torch.float32 if dtype is None else dtype
        s_plan = self._corpus_window_plan(signal[0], signal[1], channels)
        try:
            n_plan = self._corpus_window_plan(noise[0], noise[1], channels)
            try:
                s_stats = s_plan.run(signal[0], signal[2], frames, stats=True, rows=False)
                n_stats = n_plan.run(noise[0], noise[2], frames, stats=True, rows=False, spans=noise_spans)
                gains = snr_gains(s_stats, n_stats, snr_db)
                rows = s_plan.run(signal[0], signal[2], frames, dtype, gain=torch.ones_like(gains))
                n_plan.run(noise[0], noise[2], frames, dtype, out=rows, gain=gains, accumulate=True, spans=noise_spans)
                return rows, gains
            finally:
                n_plan.close()  # synchronises the context's stream first
        finally:
            s_plan.close()

    def window_levels(self, data, image_sizes, windows, frames, channels=None, spans=None):
        """The level statistics of decode_windows_mixed's rows without the rows: int64 [N, channels, 4] of (sum_sq, sum_abs,
        max_abs, count) per row, in int16 units (rmse, level_dbfs).  Nothing is stored but the table - what a rejection sampler
        asks of its candidates before it decodes the ones it keeps.  channels=None: the images share a channel count.
        spans: int64 cuda tensor [N, 2] of (num_frames, out_frame) - the levels of each window's clipped crop alone.  wide: as decode_windows_resampled."""
        plan = self._corpus_window_plan(data, image_sizes, channels)
        try:
            return plan.run(data, windows, frames, stats=True, rows=False, spans=spans)
        finally:
            plan.close()  # synchronises the context's stream first

    def resampler(self, ratios, select, wide=False):
        """A resample stage behind window decode plans (AADHip_ResamplerCreate): ratios is a list of (up, down), output rate over
        source rate, each with a bank of its own; select[stream][variant] is the index of the ratio that windows of `stream` drawn
        with `variant` take, None (or RESAMPLE_NO_BANK) for a row of zeros.  Resampler.run decodes windows at their ratios.
        wide=True: AADHip_ResamplerCreateWide - ratios of up to 32768 phases and 2 MiB of bank, such as 1600/3969 (44.1 kHz to
        16 kHz at speed 9/10); the same Resampler, the same rows."""
        ratios = [(int(u), int(d)) for u, d in ratios]
        table = np.array([[RESAMPLE_NO_BANK if v is None else int(v) for v in row] for row in select], dtype=np.int64)
        table = table.reshape(len(table), -1)
        if table.shape[1] == 0 or (table.size and (table.min() < 0 or table.max() > RESAMPLE_NO_BANK)):
            raise ValueError("select: [streams][variants] of ratio indices, at least one variant, got shape %s" % (table.shape,))
        if any(not (0 <= v < 1 << 32) for r in ratios for v in r):
            raise ValueError("ratios: (up, down) pairs of 32-bit unsigned integers, got %s" % (ratios,))
        table = np.ascontiguousarray(table, dtype=np.uint16)
        records = (AADHipResampleRatio * max(len(ratios), 1))(*[AADHipResampleRatio(u, d) for u, d in ratios])
        handle = C.c_void_p()
        name = "AADHip_ResamplerCreateWide" if wide else "AADHip_ResamplerCreate"
        _check(name, getattr(self.lib, name)(self._ctx, len(ratios), records, table.shape[0], table.shape[1], table.ctypes.data,
                                             C.byref(handle)))
        return Resampler(self, handle, ratios, table)

    def decode_windows_resampled(self, data, image_sizes, windows, frames, rate, speeds=((1, 1),), variant=None, dtype=None,
                                 channels=None, out=None, gain=None, accumulate=False, spans=None, return_stats=False, wide=False):
        """decode_windows_mixed at one output rate: every image's header names its sampling_rate, and a window of stream s drawn
        with variant v - an index into `speeds`, pairs (a, b) for the speed a / b; `variant` is an int64 cuda tensor [N], None for
        all 0 - is resampled by rate * b / (sampling_rate_s * a).  Speed 11/10 plays a stream 10 % faster: fewer output frames
        per source frame.  `frames` counts output frames, windows[:, 1] source frames as everywhere.  Streams and speeds whose
        reduced ratios agree share a bank.  dtype, channels, out: as decode_windows_mixed.
        gain / accumulate / out, spans (in output frames) and return_stats: as decode_windows_mixed, on the resampled rows
        (Resampler.run).  wide=True builds the resampler with AADHip_ResamplerCreateWide: a 44.1 kHz stream at speeds 9/10 and
        11/10 needs it (1600 phases); the default refuses such a corpus as before."""
        self._speeds(rate, speeds)
        plan = self._corpus_window_plan(data, image_sizes, channels)
        try:
            res = self._corpus_resampler(plan, rate, speeds, wide)
            try:
                return res.run(plan, data, windows, frames, variant=variant, dtype=dtype, out=out, gain=gain, accumulate=accumulate,
                               spans=spans, stats=True if return_stats else None)
            finally:
                res.close()  # synchronises the context's stream first
        finally:
            plan.close()

    def window_levels_resampled(self, data, image_sizes, windows, frames, rate, speeds=((1, 1),), variant=None, channels=None,
                                spans=None, wide=False):
        """The level statistics of decode_windows_resampled's rows without the rows: int64 [N, channels, 4] of (sum_sq, sum_abs,
        max_abs, count) per row in int16 units, count = the output frames whose centre source frame the stream had.  Nothing is
        stored but the source batch and the table.  spans: int64 cuda tensor [N, 2] of (num_frames, out_frame) in output frames -
        the levels of each window's clipped crop alone.  wide: as decode_windows_resampled."""
        self._speeds(rate, speeds)
        plan = self._corpus_window_plan(data, image_sizes, channels)
        try:
            res = self._corpus_resampler(plan, rate, speeds, wide)
            try:
                return res.run(plan, data, windows, frames, variant=variant, stats=True, rows=False, spans=spans)
            finally:
                res.close()  # synchronises the context's stream first
        finally:
            plan.close()

    def mix_windows_resampled(self, signal, noise, frames, snr_db, rate, speeds=((1, 1),), signal_variant=None, noise_variant=None,
                              dtype=None, channels=None, noise_spans=None, wide=False):
        """mix_windows at one output rate: signal, noise: each (data, image_sizes, windows) as for decode_windows_resampled, the
        same number of windows, each corpus with its own sampling rates; rate, speeds and the two variant tables as there.
        Each corpus is decoded ONCE into its int16 source batch, with statistics (Resampler.decode_source); the FIR then runs
        twice over each batch: statistics only for the levels - the noise's over noise_spans - and, with snr_gains' gains on the
        device, a STORE run of the signal and an ADD run of gain * noise into the same rows -> (rows [N, channels, frames] of
        `dtype`, float32 [N] noise gains).  No float32 batch, no elementwise pass; the roundings and the meaning of noise_spans
        (in output frames) and of the SNR are mix_windows'.  wide: as decode_windows_resampled, for both corpora."""
        torch = self.torch
        dtype = torch.float32 if dtype is None else dtype
        self._speeds(rate, speeds)
        s_plan = self._corpus_window_plan(signal[0], signal[1], channels)
        try:
            n_plan = self._corpus_window_plan(noise[0], noise[1], channels)
            try:
                ch, n_ch = int(s_plan.header.num_channels), int(n_plan.header.num_channels)
                if ch != n_ch:
                    raise ValueError("signal and noise: rows of %d and %d channels do not mix - pass channels=1 or channels=2 to bring "
                                     "both corpora to one channel count" % (ch, n_ch))
                s_res = self._corpus_resampler(s_plan, rate, speeds, wide)
                try:
                    n_res = self._corpus_resampler(n_plan, rate, speeds, wide)
                    try:
                        s_src = s_res.decode_source(s_plan, signal[0], signal[2], frames, variant=signal_variant, stats=True)
                        n_src = n_res.decode_source(n_plan, noise[0], noise[2], frames, variant=noise_variant, stats=True)
                        s_stats = s_res.run_source(s_src, frames, ch, stats=True, rows=False)
                        n_stats = n_res.run_source(n_src, frames, n_ch, stats=True, rows=False, spans=noise_spans)
                        gains = snr_gains(s_stats, n_stats, snr_db)
                        rows = s_res.run_source(s_src, frames, ch, dtype, gain=torch.ones_like(gains))
                        n_res.run_source(n_src, frames, n_ch, dtype, out=rows, gain=gains, accumulate=True, spans=noise_spans)
                        return rows, gains
                    finally:
                        n_res.close()  # synchronises the context's stream first
                finally:
                    s_res.close()
            finally:
                n_plan.close()
        finally:
            s_plan.close()

    def convolver(self, responses, delays=None):
        """A convolve stage behind window decode plans (AADHip_ConvolverCreate): responses is a list of 1-d float arrays, impulse
        responses of 1 to 32768 taps, each quantised on the host to int16 taps with a scale exponent; delays: per response the tap
        that is the direct path, None (or -1 for one response) for the largest tap.  Convolver.run reverberates windows."""
        return self._convolver(*self._responses(responses, delays))

    @staticmethod
    def _responses(responses, delays):
        """what `convolver` refuses of responses and delays, before anything is built -> (float32 arrays, ints or None)"""
        taps = [np.ascontiguousarray(np.asarray(h, dtype=np.float32).reshape(-1)) for h in responses]
        if not taps or any(not (1 <= h.size <= 32768) for h in taps):
            raise ValueError("responses: at least one, each of 1 to 32768 taps, got lengths %s" % ([int(h.size) for h in taps],))
        if delays is not None:
            delays = [-1 if d is None else int(d) for d in delays]
            if len(delays) != len(taps) or any(not (-1 <= d < h.size) for d, h in zip(delays, taps)):
                raise ValueError("delays: one per response, each a tap's index or -1 for the peak, got %s" % (delays,))
        return taps, delays

    def _convolver(self, taps, delays):
        n = len(taps)
        pointers = (C.c_void_p * n)(*[h.ctypes.data for h in taps])
        lengths = (C.c_uint32 * n)(*[h.size for h in taps])
        handle = C.c_void_p()
        _check("AADHip_ConvolverCreate",
               self.lib.AADHip_ConvolverCreate(self._ctx, n, pointers, lengths, (C.c_int32 * n)(*delays) if delays is not None else None,
                                               C.byref(handle)))
        return Convolver(self, handle, n)

    def decode_windows_reverberated(self, data, image_sizes, windows, frames, responses, response=None, delays=None, dtype=None,
                                    channels=None, out=None, gain=None, accumulate=False, spans=None, return_stats=False):
        """decode_windows_mixed with every window convolved with an impulse response: responses as for `convolver`, `response` an
        int64 cuda tensor [N] of indices into them, None for all 0.  The same response goes over every channel row; the direct path
        (delays) stays at the window's first frame, so the row is time-aligned with the dry one.  dtype, channels, out, gain /
        accumulate, spans: as decode_windows_mixed, on the reverberated rows (Convolver.run).  return_stats: -> (rows, int64
        [N, channels, 4] level statistics of the reverberated rows).  Every argument is checked before the convolver is built: a
        refused call has allocated nothing on the device but the plan's tables."""
        return self._reverberated(data, image_sizes, windows, frames, responses, response, delays, dtype, channels, out, gain,
                                  accumulate, spans, True if return_stats else None, True)

    def window_levels_reverberated(self, data, image_sizes, windows, frames, responses, response=None, delays=None, channels=None,
                                   spans=None):
        """The level statistics of decode_windows_reverberated's rows without the rows: int64 [N, channels, 4] of (sum_sq, sum_abs,
        max_abs, count) per row in int16 units - the reverberant tail counts into the sums, count = the frames of the DRY row the
        stream had.  Nothing is stored but the source batch and the table: what a rejection sampler asks of its candidates.
        spans: int64 cuda tensor [N, 2] of (num_frames, out_frame) in output frames - the levels of each window's clipped crop."""
        return self._reverberated(data, image_sizes, windows, frames, responses, response, delays, None, channels, None, None, False,
                                  spans, True, False)

    def _reverberated(self, data, image_sizes, windows, frames, responses, response, delays, dtype, channels, out, gain, accumulate,
                      spans, stats, rows):
        """decode_windows_reverberated and window_levels_reverberated: every check, then plan and convolver, then Convolver.run"""
        taps, delays = self._responses(responses, delays)
        plan = self._corpus_window_plan(data, image_sizes, channels)
        try:
            windows, checked = Convolver.check_run(self, plan, windows, frames, response, dtype, out, gain, accumulate, spans, stats, rows)
            out, stats = checked[2], checked[-1]
            conv = self._convolver(taps, delays)
            try:
                return conv.run(plan, data, windows, frames, response=response, dtype=dtype, out=out, gain=gain,
                                accumulate=accumulate, spans=spans, stats=stats, rows=rows)
            finally:
                conv.close()  # synchronises the context's stream first
        finally:
            plan.close()

    def mix_windows_reverberated(self, signal, noise, frames, snr_db, responses, response=None, delays=None, noise_responses=None,
                                 noise_response=None, noise_delays=None, dtype=None, channels=None, noise_spans=None):
        """mix_windows with the signal convolved with a room response, the SNR measured against the REVERBERANT signal: signal,
        noise: each (data, image_sizes, windows) as for decode_windows_reverberated, the same number of windows; responses,
        response, delays: the signal's, as there.  The signal corpus is decoded ONCE into its int16 source batch, with statistics
        (Convolver.decode_source); the FIR then runs twice over it: statistics only for the levels and a STORE run with a gain of
        ones.  noise_responses=None: the noise is dry - its plan's own statistics-only run (over noise_spans) and ADD run, exactly
        as in mix_windows.  Else the noise gets a convolver of its own (noise_responses, noise_response, noise_delays), one decode
        and two FIR runs, as in mix_windows_resampled -> (rows [N, channels, frames] of `dtype`, float32 [N] noise gains).  No
        float32 batch, no elementwise pass; the roundings and the meaning of noise_spans (in output frames) and of the SNR are
        mix_windows'.  Every argument is checked before anything but the plans' tables is built on the device."""
        torch = self.torch
        dtype = torch.float32 if dtype is None else dtype
        taps, delays = self._responses(responses, delays)
        wet_noise = noise_responses is not None
        if wet_noise:
            n_taps, n_delays = self._responses(noise_responses, noise_delays)
        elif noise_response is not None or noise_delays is not None:
            raise ValueError("noise_response / noise_delays: the noise has no responses - pass noise_responses")
        s_plan = self._corpus_window_plan(signal[0], signal[1], channels)
        try:
            n_plan = self._corpus_window_plan(noise[0], noise[1], channels)
            try:
                ch, n_ch = int(s_plan.header.num_channels), int(n_plan.header.num_channels)
                if ch != n_ch:
                    raise ValueError("signal and noise: rows of %d and %d channels do not mix - pass channels=1 or channels=2 to bring "
                                     "both corpora to one channel count" % (ch, n_ch))
                # the four runs' arguments, before a convolver exists: levels and STORE of the signal, levels and ADD of the noise
                _fir_sample_type(torch, Convolver.WHAT, dtype)
                s_win = self.window_table(signal[2], True)
                n = int(s_win.shape[0])
                if response is not None:
                    self.tensor("response", response, torch.int64, n, shape=(n,), contiguous=True)
                if dtype == torch.int16:
                    raise ValueError("gain / accumulate: float rows only (torch.float32, torch.float16, torch.bfloat16), not torch.int16")
                n_win = self.window_table(noise[2], True, name="noise windows", rows=n)
                if noise_spans is not None:
                    noise_spans = self.window_table(noise_spans, True, name="noise_spans", rows=n)
                if wet_noise and noise_response is not None:
                    self.tensor("noise_response", noise_response, torch.int64, n, shape=(n,), contiguous=True)
                s_conv = self._convolver(taps, delays)
                try:
                    s_src = s_conv.decode_source(s_plan, signal[0], s_win, frames, response=response, stats=True)
                    s_stats = s_conv.run_source(s_src, frames, ch, stats=True, rows=False)
                    if not wet_noise:
                        n_stats = n_plan.run(noise[0], n_win, frames, stats=True, rows=False, spans=noise_spans)
                        gains = snr_gains(s_stats, n_stats, snr_db)
                        rows = s_conv.run_source(s_src, frames, ch, dtype, gain=torch.ones_like(gains))
                        n_plan.run(noise[0], n_win, frames, dtype, out=rows, gain=gains, accumulate=True, spans=noise_spans)
                        return rows, gains
                    n_conv = self._convolver(n_taps, n_delays)
                    try:
                        n_src = n_conv.decode_source(n_plan, noise[0], n_win, frames, response=noise_response, stats=True)
                        n_stats = n_conv.run_source(n_src, frames, n_ch, stats=True, rows=False, spans=noise_spans)
                        gains = snr_gains(s_stats, n_stats, snr_db)
                        rows = s_conv.run_source(s_src, frames, ch, dtype, gain=torch.ones_like(gains))
                        n_conv.run_source(n_src, frames, n_ch, dtype, out=rows, gain=gains, accumulate=True, spans=noise_spans)
                        return rows, gains
                    finally:
                        n_conv.close()  # synchronises the context's stream first
                finally:
                    s_conv.close()
            finally:
                n_plan.close()
        finally:
            s_plan.close()

    # ---- spectrogram ------------------------------------------------------------------------------------------------------------
    def spectrogram(self, n_fft, hop, win_length=None, window=None, filters=None):
        """A spectrogram stage over int16 rows (AADHip_SpectrogramCreate, include/aad_hip.h "spectrogram"): n_fft up to 4096, hop
        >= 1, win_length (None: n_fft) up to n_fft; window: 1-d float array [win_length], None for the periodic Hann window
        computed in float64 and rounded to float32; filters: float array [M, n_fft // 2 + 1] such as mel_filters gives, None for
        the power spectrum itself.  Spectrogram.run turns rows into [.., F, M] energies, or [.., F, B] powers."""
        return self._spectrogram(*_spectrogram_arguments(n_fft, hop, win_length, window, filters))

    def _spectrogram(self, n_fft, hop, win_length, window, filters):
        handle = C.c_void_p()
        m = 0 if filters is None else int(filters.shape[0])
        _check("AADHip_SpectrogramCreate",
               self.lib.AADHip_SpectrogramCreate(self._ctx, n_fft, win_length, hop, window.ctypes.data, m,
                                                 filters.ctypes.data if m else None, C.byref(handle)))
        return Spectrogram(self, handle, n_fft, hop, win_length, m)

    def mel_windows(self, data, image_sizes, windows, frames, n_fft, hop, filters, channels=None, win_length=None, window=None):
        """decode_windows_mixed's int16 rows through a spectrogram stage -> float32 [N, C, F, M] (M = n_fft // 2 + 1 powers for
        filters=None): data, image_sizes, windows, frames, channels as decode_windows_mixed; n_fft, hop, filters, win_length,
        window as `spectrogram`.  F = 1 + (frames - win_length) // hop.  The int16 batch is the one temporary.  Every argument is
        checked before anything is built."""
        args = _spectrogram_arguments(n_fft, hop, win_length, window, filters)
        frames = int(frames)
        if frames < args[2]:
            raise ValueError("frames: %d is below the window's %d - such a row has no frame" % (frames, args[2]))
        windows = self.window_table(windows, True)
        plan = self._corpus_window_plan(data, image_sizes, channels)
        try:
            spec = self._spectrogram(*args)
            try:
                return spec.run(plan.run(data, windows, frames, self.torch.int16))
            finally:
                spec.close()  # synchronises the context's stream first
        finally:
            plan.close()

    def mel_mix_windows(self, signal, noise, frames, snr_db, n_fft, hop, filters, channels=None, win_length=None, window=None,
                        noise_spans=None):
        """The features of a noisy batch at a chosen SNR - mix_windows and mel_windows in one, without the float32 rows between
        them: signal, noise, snr_db, channels, noise_spans as mix_windows; n_fft, hop, filters, win_length, window as
        `spectrogram`.  Two statistics-only runs give the levels - the noise's over its spans - snr_gains the noise gains, two
        decodes the int16 rows of signal and noise, and ONE Spectrogram.run_mix sums them per element as
        clamp(rint(signal + fl32(gain * noise))) while it stages them -> (float32 [N, C, F, M], float32 [N] noise gains).  The two
        int16 batches are the only temporaries.  Every argument is checked before anything is built."""
        torch = self.torch
        args = _spectrogram_arguments(n_fft, hop, win_length, window, filters)
        frames = int(frames)
        if frames < args[2]:
            raise ValueError("frames: %d is below the window's %d - such a row has no frame" % (frames, args[2]))
        s_windows = self.window_table(signal[2], True)
        n_windows = self.window_table(noise[2], True, rows=int(s_windows.shape[0]))
        if noise_spans is not None:
            noise_spans = self.window_table(noise_spans, True, name="spans", rows=int(s_windows.shape[0]))
        s_plan = self._corpus_window_plan(signal[0], signal[1], channels)
        try:
            n_plan = self._corpus_window_plan(noise[0], noise[1], channels)
            try:
                spec = self._spectrogram(*args)
                try:
                    s_stats = s_plan.run(signal[0], s_windows, frames, stats=True, rows=False)
                    n_stats = n_plan.run(noise[0], n_windows, frames, stats=True, rows=False, spans=noise_spans)
                    gains = snr_gains(s_stats, n_stats, snr_db)
                    s_rows = s_plan.run(signal[0], s_windows, frames, torch.int16)
                    n_rows = n_plan.run(noise[0], n_windows, frames, torch.int16)
                    return spec.run_mix(s_rows, n_rows, other_gain=gains, spans=noise_spans), gains
                finally:
                    spec.close()  # synchronises the context's stream first
            finally:
                n_plan.close()
        finally:
            s_plan.close()

    @staticmethod
    def _speeds(rate, speeds):
        """what the resampled calls refuse of rate and speeds, before anything is built -> the speeds as pairs of ints"""
        speeds = [(int(a), int(b)) for a, b in speeds]
        if int(rate) <= 0 or not speeds or any(a <= 0 or b <= 0 for a, b in speeds):
            raise ValueError("rate and speeds: positive integers, at least one speed; got rate %r, speeds %r" % (rate, speeds))
        return speeds

    def _corpus_resampler(self, plan, rate, speeds, wide=False):
        """the resampler of a corpus plan at one output rate: per stream and speed (a, b) the ratio rate * b / (sampling_rate * a),
        equal reduced ratios sharing a bank"""
        from math import gcd
        speeds = self._speeds(rate, speeds)
        ratios, select = [], []
        for h in plan.headers:
            if h.sampling_rate == 0:
                raise ValueError("an image's header has sampling_rate 0: no ratio to resample it by")
            row = []
            for a, b in speeds:
                up, down = int(rate) * b, int(h.sampling_rate) * a
                g = gcd(up, down)
                r = (up // g, down // g)
                if r not in ratios:
                    ratios.append(r)
                row.append(ratios.index(r))
            select.append(row)
        return self.resampler(ratios, select, wide) if wide else self.resampler(ratios, select)

    def _corpus_window_plan(self, data, image_sizes, channels):
        """the window decode plan over the images in the rows of `data`: mixed-format, or channel-mix when `channels` is given"""
        sizes = self.image_rows("data", data, image_sizes)
        s = int(data.shape[0])
        if int(data.shape[1]) < 31:
            raise ApiError("parse_header", AADApiResult.INVALID_FORMAT)
        heads = data[:, :31].cpu().numpy()
        headers = [parse_header(bytes(row)) for row in heads]
        d = np.zeros(s, dtype=STREAM_DESC_DTYPE)
        d["data_offset"] = np.arange(s, dtype=np.uint64) * np.uint64(data.stride(0))
        d["data_size"] = sizes
        d["num_samples"] = [h.num_samples for h in headers]
        return self.mixed_window_decode_plan(headers, d, True) if channels is None \
            else self.channel_mix_window_decode_plan(headers, d, channels, True)

    # ---- reconstruction modes (the reference CLI's -r / -g / -c, src/main.c:275-503) ----------
    def reconstruct_uniform(self, pcm, param, residual=False, want_stats=True, segment_blocks=None, warmup_blocks=0):
        """pcm: int16 cuda tensor [streams, samples, channels] -> (out int16 tensor of the same
        shape, stats float64 tensor [streams, 3] = RMSE, MSD, MaxAE or None).  Encode, decode and
        the comparison run back to back on the device; the images stay in a scratch tensor.
        segment_blocks / warmup_blocks: over the images of a segmented encode (see encode_plan)."""
        torch = self.torch
        streams, samples, ch = self.interleaved_input("reconstruct_uniform", pcm, param)
        size = self.encoded_size(param, samples)
        if size == 0:
            raise ApiError("AADHip_CalculateEncodedSize", AADApiResult.INVALID_FORMAT)
        stride = _round_up(size, 16)
        d = np.zeros(streams, dtype=STREAM_DESC_DTYPE)
        i = np.arange(streams, dtype=np.uint64)
        d["pcm_offset"] = i * np.uint64(samples * ch)
        d["data_offset"] = i * np.uint64(stride)
        d["data_size"] = stride
        d["num_samples"] = samples
        plan = C.c_void_p()
        if segment_blocks is None:
            _check("AADHip_ReconstructPlanCreate",
                   self.lib.AADHip_ReconstructPlanCreate(self._ctx, C.byref(param), streams, d.ctypes.data, C.byref(plan)))
        else:
            seg = AADHipSegmentation(int(segment_blocks), int(warmup_blocks))
            _check("AADHip_SegmentedReconstructPlanCreate",
                   self.lib.AADHip_SegmentedReconstructPlanCreate(self._ctx, C.byref(param), C.byref(seg), streams, d.ctypes.data,
                                                                  C.byref(plan)))
        try:
            images = torch.empty((streams, stride), dtype=torch.uint8, device=pcm.device)
            out = torch.empty_like(pcm)
            stats = torch.empty((streams, 3), dtype=torch.float64, device=pcm.device) if want_stats else None
            cur = self._enter()
            _check("AADHip_ReconstructPlanRun",
                   self.lib.AADHip_ReconstructPlanRun(plan, pcm.data_ptr(), images.data_ptr(), out.data_ptr(),
                                                      RECONSTRUCT_RESIDUAL if residual else RECONSTRUCT_DECODED,
                                                      stats.data_ptr() if want_stats else None))
            self._exit(cur)
        finally:
            self.lib.AADHip_ReconstructPlanDestroy(plan)  # synchronises the stream first
        return out, stats

    def reconstruct_host(self, pcm_list, param, residual=False, want_pcm=True, want_stats=True, segment_blocks=None, warmup_blocks=0):
        """pcm_list: int16 arrays [samples, channels] -> (list of int16 arrays or None,
        ERROR_STATS_DTYPE array [streams] or None) through AADHip_ReconstructBatch, or with segment_blocks
        AADHip_SegmentedReconstructBatch (the images of a segmented encode, see encode_plan)."""
        n = len(pcm_list)
        pcm_list = _host_pcm("reconstruct_host", pcm_list, param)
        nsamp = np.array([p.shape[0] for p in pcm_list], dtype=np.uint32)
        outs = [np.zeros_like(p) for p in pcm_list] if want_pcm else None
        stats = np.zeros(n, dtype=ERROR_STATS_DTYPE) if want_stats else None
        pp = (C.c_void_p * n)(*[p.ctypes.data for p in pcm_list])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs]) if want_pcm else None
        kind = RECONSTRUCT_RESIDUAL if residual else RECONSTRUCT_DECODED
        sp = stats.ctypes.data if want_stats else None
        if segment_blocks is None:
            _check("AADHip_ReconstructBatch",
                   self.lib.AADHip_ReconstructBatch(self._ctx, C.byref(param), n, pp, nsamp.ctypes.data, kind, op, sp))
        else:
            seg = AADHipSegmentation(int(segment_blocks), int(warmup_blocks))
            _check("AADHip_SegmentedReconstructBatch",
                   self.lib.AADHip_SegmentedReconstructBatch(self._ctx, C.byref(param), C.byref(seg), n, pp, nsamp.ctypes.data,
                                                             kind, op, sp))
        return outs, stats

    # ---- host-memory batches ----------------------------------------------------------------
    def encode_host(self, pcm_list, param, state=None, segment_blocks=None, warmup_blocks=0):
        """pcm_list: list of int16 arrays [samples, channels] -> list of bytes.  state: optional
        LANE_STATE_DTYPE array [streams * channels], updated in place.  segment_blocks / warmup_blocks:
        a segmented encode (AADHip_SegmentedEncodeBatch, see encode_plan), which takes no state."""
        if state is not None and segment_blocks is not None:
            raise ValueError("a segmented encode starts from fresh encoders: state and segment_blocks exclude each other")
        n = len(pcm_list)
        pcm_list = _host_pcm("encode_host", pcm_list, param)
        if state is not None and (not isinstance(state, np.ndarray) or state.dtype != LANE_STATE_DTYPE or state.ndim != 1
                                  or len(state) != n * param.num_channels or not state.flags["C_CONTIGUOUS"]):
            raise ValueError("encode_host: state: a contiguous LANE_STATE_DTYPE array [%d] (streams * channels) is needed, got %s"
                             % (n * param.num_channels, "%s %s" % (state.dtype, state.shape) if isinstance(state, np.ndarray)
                                else type(state).__name__))
        nsamp = np.array([p.shape[0] for p in pcm_list], dtype=np.uint32)
        caps = np.array([max(self.encoded_size(param, int(s)), 64) for s in nsamp], dtype=np.uint64)
        outs = [np.zeros(int(c), dtype=np.uint8) for c in caps]
        sizes = np.zeros(n, dtype=np.uint64)
        pp = (C.c_void_p * n)(*[p.ctypes.data for p in pcm_list])
        op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        if segment_blocks is None:
            sp = state.ctypes.data if state is not None else None
            _check("AADHip_EncodeBatch",
                   self.lib.AADHip_EncodeBatch(self._ctx, C.byref(param), n, pp, nsamp.ctypes.data, op,
                                               caps.ctypes.data, sizes.ctypes.data, sp))
        else:
            seg = AADHipSegmentation(int(segment_blocks), int(warmup_blocks))
            _check("AADHip_SegmentedEncodeBatch",
                   self.lib.AADHip_SegmentedEncodeBatch(self._ctx, C.byref(param), C.byref(seg), n, pp, nsamp.ctypes.data, op,
                                                        caps.ctypes.data, sizes.ctypes.data))
        return [o[: int(s)].tobytes() for o, s in zip(outs, sizes)]

    def decode_host(self, images):
        """images: list of bytes (one format) -> list of int16 arrays [samples, channels]"""
        n = len(images)
        bufs = [np.frombuffer(b, dtype=np.uint8) for b in images]
        heads = [parse_header(bytes(b[:31])) for b in images]
        pcms = [np.zeros((h.num_samples, h.num_channels), dtype=np.int16) for h in heads]
        sizes = np.array([len(b) for b in bufs], dtype=np.uint64)
        caps = np.array([h.num_samples for h in heads], dtype=np.uint32)
        got = np.zeros(n, dtype=np.uint32)
        dp = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        pp = (C.c_void_p * n)(*[p.ctypes.data for p in pcms])
        _check("AADHip_DecodeBatch",
               self.lib.AADHip_DecodeBatch(self._ctx, n, dp, sizes.ctypes.data, pp, caps.ctypes.data, got.ctypes.data))
        return pcms


def _host_pcm(what, pcm_list, param):
    """the host entry points' input: int16 arrays [samples, channels] of the parameter's channel count (mono: 1-D is fine too),
    contiguous - the C call reads samples * channels values behind each pointer"""
    ch = int(param.num_channels)
    out = []
    for i, p in enumerate(pcm_list):
        p = np.ascontiguousarray(p, dtype=np.int16)
        if not ((p.ndim == 2 and p.shape[1] == ch) or (p.ndim == 1 and ch == 1)):
            raise ValueError("%s: pcm_list[%d]: an array [samples, %d] is needed (the parameter's channels%s), got shape %s"
                             % (what, i, ch, "; mono may be 1-D" if ch == 1 else "", p.shape))
        out.append(p)
    return out


def _stats_f64(stats):
    """the fields of an int64 [..., 4] statistics tensor as float64: int64 -> float64 directly, never through float32"""
    import torch
    if stats.dtype != torch.int64 or stats.shape[-1] != 4:
        raise ValueError("stats: an int64 tensor [..., 4] (sum_sq, sum_abs, max_abs, count)")
    return stats.to(torch.float64).unbind(-1)


def rmse(stats):
    """sqrt(sum_sq / count) per row of an int64 [..., 4] statistics tensor, float64, in int16 units; NaN for an empty row"""
    sum_sq, _, _, count = _stats_f64(stats)
    return (sum_sq / count).sqrt()


def level_dbfs(stats):
    """20 log10(rmse / 32768) per row of an int64 [..., 4] statistics tensor, float64: the row's RMS level against full scale;
    -inf for an all-zero or empty row"""
    import torch
    sum_sq, _, _, count = _stats_f64(stats)
    mean = torch.where(count == 0, torch.zeros_like(sum_sq), sum_sq / count.clamp(min=1.0))
    return 20.0 * (mean.sqrt() / 32768.0).log10()


def snr_gains(signal_stats, noise_stats, snr_db):
    """The noise gains that put each window's noise snr_db below its signal: from two int64 [N, C, 4] statistics tables (the two
    may differ in C) float32 [N] of sqrt(P_s / P_n) * 10^(-snr_db / 20), P = the sum of sum_sq over the window's rows divided by
    the sum of count, computed in float64; 0 where either power or either count is 0.  snr_db: a number or a tensor [N].
    Stays on the tables' device, no synchronisation."""
    import torch
    s_sq, _, _, s_count = _stats_f64(signal_stats)
    n_sq, _, _, n_count = _stats_f64(noise_stats)
    s_sq, s_count, n_sq, n_count = s_sq.sum(-1), s_count.sum(-1), n_sq.sum(-1), n_count.sum(-1)
    p_s, p_n = s_sq / s_count.clamp(min=1.0), n_sq / n_count.clamp(min=1.0)
    silent = (s_sq == 0) | (n_sq == 0) | (s_count == 0) | (n_count == 0)
    scale = torch.pow(10.0, -snr_db.to(device=s_sq.device, dtype=torch.float64) / 20.0) if torch.is_tensor(snr_db) \
        else 10.0 ** (-float(snr_db) / 20.0)  # a number never becomes a tensor: no copy to the device
    g = (p_s / torch.where(silent, torch.ones_like(p_n), p_n)).sqrt() * scale
    return torch.where(silent, torch.zeros_like(g), g).to(torch.float32)


def snr_db(stats, signal_sum_sq):
    """10 log10(signal_sum_sq / sum_sq) per row, float64; signal_sum_sq: the rows' signal power in the same int16 units (sum of
    squared samples, any integer or float dtype).  An empty row gives NaN, a zero error +inf."""
    import torch
    sum_sq, _, _, count = _stats_f64(stats)
    signal = torch.as_tensor(signal_sum_sq, device=stats.device).to(torch.float64)
    ratio = torch.where(sum_sq == 0, torch.full_like(sum_sq, float("inf")), signal / sum_sq)
    return torch.where(count == 0, torch.full_like(sum_sq, float("nan")), 10.0 * ratio.log10())


def select_least_bits(snr_by_bits, min_snr_db):
    """snr_by_bits: the [N, C] SNR tensors of 2, 3 and 4 bits -> int64 [N]: the fewest bits at which every channel of a stream
    reaches min_snr_db, 0 where none does (a NaN - an empty row - meets no bound)"""
    import torch
    best = torch.zeros(snr_by_bits[0].shape[0], dtype=torch.int64, device=snr_by_bits[0].device)
    for bits, snr in reversed(list(zip((2, 3, 4), snr_by_bits))):
        best = torch.where((snr >= min_snr_db).all(dim=-1), torch.full_like(best, bits), best)
    return best


class EncodePlan:
    def __init__(self, engine, handle, param, descs):
        self.engine, self.handle, self.param, self.descs = engine, handle, param, descs
        self.image_size = self.stride = None
        self.segmented = False
        self._extents, self._memo = {}, {}  # per run argument: the elements a run touches; the layout that passed the check last

    def extent(self, kind, **layout):
        """run_extent of this plan's table, computed once (the table never changes)"""
        if kind not in self._extents:
            self._extents[kind] = run_extent(kind, self.descs, self.param.num_channels, **layout)
        return self._extents[kind]

    def run(self, pcm, data, state=None, ordered=True):
        """pcm: int16 cuda tensor that holds every stream's frames at its pcm_offset, data: uint8 cuda tensor that holds every
        image's data_size bytes at its data_offset (both counted from data_ptr(), stride(-1) == 1), state: int32 cuda tensor
        [lanes, 10] or None.
        ordered=False: launch on the engine's stream without ordering it against torch's current stream
        (the caller orders the streams itself, with events - see bench.py's pipelined step)."""
        if state is not None and self.segmented:
            raise ValueError("a segmented encode plan takes no state")
        e = self.engine
        e.tensor("pcm", pcm, e.torch.int16, self.extent("interleaved"), rows_in_place=True, memo=self._memo)
        e.tensor("data", data, e.torch.uint8, self.extent("images"), rows_in_place=True, memo=self._memo)
        e.state_tensor(state, len(self.descs), self.param.num_channels, self._memo)
        sp = state.data_ptr() if state is not None else None
        cur = self.engine._enter() if ordered else None
        _check("AADHip_EncodePlanRun",
               self.engine.lib.AADHip_EncodePlanRun(self.handle, pcm.data_ptr(), data.data_ptr(), sp))
        if ordered:
            self.engine._exit(cur)

    def close(self):
        if self.handle:
            self.engine.lib.AADHip_EncodePlanDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlanarEncodePlan(EncodePlan):
    def __init__(self, engine, handle, param, descs, dtype, channel_stride):
        super().__init__(engine, handle, param, descs)
        self.dtype, self.channel_stride = dtype, channel_stride

    def run(self, x, data, state=None, ordered=True):
        """x: cuda tensor of the plan's dtype whose data_ptr() the table's pcm_offsets count from (elements; it spans every row the
        table names), data: uint8 cuda tensor, state: int32 cuda tensor [lanes, 10] or None; ordered as EncodePlan.run"""
        if state is not None and self.segmented:
            raise ValueError("a segmented encode plan takes no state")
        e = self.engine
        e.tensor("x", x, self.dtype, self.extent("planar", channel_stride=self.channel_stride), rows_in_place=True, memo=self._memo)
        e.tensor("data", data, e.torch.uint8, self.extent("images"), rows_in_place=True, memo=self._memo)
        e.state_tensor(state, len(self.descs), self.param.num_channels, self._memo)
        sp = state.data_ptr() if state is not None else None
        cur = self.engine._enter() if ordered else None
        _check("AADHip_PlanarEncodePlanRun",
               self.engine.lib.AADHip_PlanarEncodePlanRun(self.handle, x.data_ptr(), data.data_ptr(), sp))
        if ordered:
            self.engine._exit(cur)


class PlanarReconstructPlan(EncodePlan):
    def __init__(self, engine, handle, param, descs, dtype, out_dtype, channel_stride, out_stream_stride, out_channel_stride):
        super().__init__(engine, handle, param, descs)
        self.dtype, self.out_dtype, self.channel_stride = dtype, out_dtype, channel_stride
        self.out_stream_stride, self.out_channel_stride = out_stream_stride, out_channel_stride

    def run(self, x, data, out, state=None, ordered=True, stats=None):
        """x: cuda rows of the plan's dtype (the table's pcm_offsets count from x.data_ptr()), data: uint8 cuda tensor for the images,
        out: cuda tensor of the plan's out_dtype (the output strides count from out.data_ptr()), state as EncodePlan.run.
        stats: a contiguous int64 cuda tensor [N, C, 4] that the same run fills with the rows' error statistics
        (AADHip_PlanarReconstructPlanRunStats; its contents before the run do not matter); with it, out=None writes no rows."""
        if out is None and stats is None:
            raise ValueError("out=None needs stats")
        if state is not None and self.segmented:
            raise ValueError("a segmented encode plan takes no state")
        e, n, ch = self.engine, len(self.descs), self.param.num_channels
        e.tensor("x", x, self.dtype, self.extent("planar", channel_stride=self.channel_stride), rows_in_place=True, memo=self._memo)
        e.tensor("data", data, e.torch.uint8, self.extent("images"), rows_in_place=True, memo=self._memo)
        if out is not None:
            e.tensor("out", out, self.out_dtype, self.extent("planar_out", stream_stride=self.out_stream_stride,
                                                             channel_stride=self.out_channel_stride), rows_in_place=True, memo=self._memo)
        if stats is not None:
            e.tensor("stats", stats, e.torch.int64, self.extent("stats", rows=n), shape=(n, ch, 4), contiguous=True, memo=self._memo)
        e.state_tensor(state, n, ch, self._memo)
        sp = state.data_ptr() if state is not None else None
        cur = self.engine._enter() if ordered else None
        if stats is not None:
            _check("AADHip_PlanarReconstructPlanRunStats",
                   self.engine.lib.AADHip_PlanarReconstructPlanRunStats(self.handle, x.data_ptr(), data.data_ptr(),
                                                                        out.data_ptr() if out is not None else None, sp, stats.data_ptr()))
        else:
            _check("AADHip_PlanarReconstructPlanRun",
                   self.engine.lib.AADHip_PlanarReconstructPlanRun(self.handle, x.data_ptr(), data.data_ptr(), out.data_ptr(), sp))
        if ordered:
            self.engine._exit(cur)


class WindowReconstructPlan(EncodePlan):
    def __init__(self, engine, handle, param, source_table, dtype, channel_stride):
        super().__init__(engine, handle, param, source_table)
        self.dtype, self.channel_stride = dtype, channel_stride

    def run(self, x, windows, frames, out=None, dtype=None, data=None, stats=None, ordered=True):
        """x: the corpus, a cuda tensor of the plan's dtype (the source table's pcm_offsets count from x.data_ptr()); windows: int64
        cuda tensor [N, 2] of (stream, first_frame), never read on the host; frames: T.  Returns the rows.
        out: None allocates a contiguous [N, C, T] tensor of `dtype` (default: the plan's dtype); False writes no rows; else a
        torch.int16 or torch.float32 cuda tensor [N, C, T] with out.stride(-1) == 1, written in place, every element of it.
        data: None (the images stay in the engine's scratch) or a uint8 cuda tensor [N, stride >= the image of T frames];
        stats: None or a contiguous int64 cuda tensor [N, C, 4].  At least one of the three.  ordered as EncodePlan.run."""
        e, torch = self.engine, self.engine.torch
        e.tensor("x", x, self.dtype, self.extent("planar", channel_stride=self.channel_stride), rows_in_place=True)
        windows = e.window_table(windows, ordered)
        n, ch, frames = int(windows.shape[0]), int(self.param.num_channels), int(frames)
        if out is None:
            out = torch.empty((n, ch, frames), dtype=self.dtype if dtype is None else dtype, device=windows.device)
        elif out is False:
            out = None
        if out is not None:  # its own strides go to the library, so its own span is what the run writes
            e.tensor("out", out, (torch.int16, torch.float32), shape=(n, ch, frames), rows_in_place=True)
            if dtype is not None and out.dtype != dtype:
                raise ValueError("out: dtype %s was asked for, the tensor has %s" % (dtype, out.dtype))
        if out is None and data is None and stats is None:
            raise ValueError("nothing to write: out, data and stats are all absent")
        image_stride = 0
        if data is not None:
            e.tensor("data", data, torch.uint8, shape=(n, None), rows_in_place=True)
            if int(data.shape[1]) < e.encoded_size(self.param, frames):
                raise ValueError("data: rows of %d bytes, the image of %d frames has %d"
                                 % (int(data.shape[1]), frames, e.encoded_size(self.param, frames)))
            image_stride = int(data.stride(0))
        if stats is not None:
            e.tensor("stats", stats, torch.int64, run_extent("stats", rows=n, channels=ch), shape=(n, ch, 4), contiguous=True)
        output = None
        if out is not None:
            output = AADHipPlanarOutput(SAMPLE_FLOAT32 if out.dtype == torch.float32 else SAMPLE_INT16, 0,
                                        int(out.stride(0)) if n > 1 else ch * frames, int(out.stride(1)) if ch > 1 else frames)
        cur = self.engine._enter() if ordered else None
        _check("AADHip_WindowReconstructPlanRun",
               self.engine.lib.AADHip_WindowReconstructPlanRun(
                   self.handle, x.data_ptr(), n, windows.data_ptr(), frames, image_stride, data.data_ptr() if data is not None else None,
                   C.byref(output) if output is not None else None, out.data_ptr() if out is not None else None,
                   stats.data_ptr() if stats is not None else None))
        if ordered:
            self.engine._exit(cur)
        return out

    def close(self):
        if self.handle:
            self.engine.lib.AADHip_WindowReconstructPlanDestroy(self.handle)
            self.handle = None


class DecodePlan:
    def __init__(self, engine, handle, header, descs):
        self.engine, self.handle, self.header, self.descs = engine, handle, header, descs
        self._memo = {}
        self.data_extent = run_extent("images", descs)
        self.pcm_extent = run_extent("interleaved", descs, header.num_channels)

    def run(self, data, pcm, ordered=True):
        """data: uint8 cuda tensor that holds every image's data_size bytes at its data_offset, pcm: int16 cuda tensor that holds
        every stream's num_samples frames at its pcm_offset (both counted from data_ptr(), stride(-1) == 1); ordered as EncodePlan.run"""
        e = self.engine
        e.tensor("data", data, e.torch.uint8, self.data_extent, rows_in_place=True, memo=self._memo)
        e.tensor("pcm", pcm, e.torch.int16, self.pcm_extent, rows_in_place=True, memo=self._memo)
        cur = self.engine._enter() if ordered else None
        _check("AADHip_DecodePlanRun",
               self.engine.lib.AADHip_DecodePlanRun(self.handle, data.data_ptr(), pcm.data_ptr()))
        if ordered:
            self.engine._exit(cur)

    def close(self):
        if self.handle:
            self.engine.lib.AADHip_DecodePlanDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowDecodePlan:
    def __init__(self, engine, handle, header, descs):
        self.engine, self.handle, self.header, self.descs = engine, handle, header, descs
        self._memo = {}
        self.data_extent = run_extent("images", descs)

    def run(self, data, windows, frames, dtype=None, out=None, ordered=True, stats=None, rows=True, gain=None, accumulate=False,
            spans=None):
        """data: uint8 cuda tensor of the images; windows: int64 cuda tensor [N, 2] of (stream, first_frame) ->
        `out` ([N, channels, frames] of dtype torch.float32 - sample / 32768 - or torch.int16; allocated when None).
        dtype torch.float16 / torch.bfloat16: the float32 row rounded once to nearest even, bit for bit row_float32.to(dtype),
        from the kernel's own stores - what a model under autocast takes without a cast pass.
        Asynchronous on the engine's stream, ordered against torch's current one; the windows stay on the device.
        stats (AADHip_WindowDecodePlanRunStats): True, or a contiguous cuda int64 tensor [N, channels, 4] - the exact level
        statistics of every row (sum_sq, sum_abs, max_abs in int16 units, count = the frames the stream had), from the same
        kernels -> (out, stats).  rows=False: statistics only, no row is written -> stats.
        gain (AADHip_WindowDecodePlanRunGain): a contiguous float32 cuda tensor [N], one gain per window for all its rows - the
        float rows hold fl32(gain * row_float32) rounded once to `dtype`; it stays on the device and must stay alive until the run
        is done (nothing is copied, so ordered=False needs no more than that).  accumulate=True: the run ADDS into `out`
        (needed then) instead of storing - (out.float() + gain[:, None, None] * row_float32).to(dtype), a multiply and an add,
        two roundings; without `gain` every gain is 1.  Not for torch.int16, and not together with stats: the levels come first,
        from a statistics-only run (stats=True, rows=False), and the gains from them (snr_gains).
        spans (AADHip_WindowDecodePlanRunPlaced / ...RunPlacedStats): an int64 cuda tensor [N, 2] of (num_frames, out_frame) by
        the rules of `windows`, never read on the host.  Window w's crop is clipped to Le = 0 if out_frame >= frames, else
        min(num_frames, frames - out_frame), and lands at out[w, :, out_frame:out_frame + Le].  With rows - float dtypes only,
        `gain` and `accumulate` as above - the rest of the row becomes +0, or under accumulate=True stays untouched;
        with stats=True, rows=False the levels and `count` are those of the Le frames.  Not for torch.int16, and not for rows and
        statistics together."""
        torch = self.engine.torch
        dtype = torch.float32 if dtype is None else dtype
        gained = gain is not None or bool(accumulate)
        placed = spans is not None
        if placed:
            if not (stats is None or stats is False) and rows:
                raise ValueError("spans: no run with both rows and statistics - take the levels from a statistics-only run "
                                 "(stats=True, rows=False, spans=...), then the rows")
            if rows and dtype == torch.int16:
                raise ValueError("spans: float rows only (torch.float32, torch.float16, torch.bfloat16), not torch.int16")
        kinds = {torch.float32: SAMPLE_FLOAT32, torch.int16: SAMPLE_INT16, torch.float16: SAMPLE_FLOAT16, torch.bfloat16: SAMPLE_BFLOAT16}
        if dtype not in kinds:
            raise ValueError("window decode writes torch.float32, torch.int16, torch.float16 or torch.bfloat16, not %s" % dtype)
        e = self.engine
        e.tensor("data", data, torch.uint8, self.data_extent, rows_in_place=True, memo=self._memo)
        windows = e.window_table(windows, ordered)
        n, ch, frames = int(windows.shape[0]), int(self.header.num_channels), int(frames)
        if placed:
            spans = e.window_table(spans, ordered, name="spans", rows=n)
        if gained:
            if dtype == torch.int16:
                raise ValueError("gain / accumulate: float rows only (torch.float32, torch.float16, torch.bfloat16), not torch.int16")
            if not (stats is None or stats is False) or not rows:
                raise ValueError("gain / accumulate: no statistics variant - take the levels first from a statistics-only run "
                                 "(stats=True, rows=False), then run with the gains")
            if accumulate and out is None:
                raise ValueError("accumulate=True adds into `out`: pass the rows to add to")
            if gain is not None:
                e.tensor("gain", gain, torch.float32, n, shape=(n,), contiguous=True)
        if stats is None or stats is False:
            stats = None
            if not rows:
                raise ValueError("rows=False is a statistics-only run: pass stats=True or a table")
        elif stats is True:
            stats = torch.empty((n, ch, 4), dtype=torch.int64, device=windows.device)
        else:
            e.tensor("stats", stats, torch.int64, run_extent("stats", rows=n, channels=ch), shape=(n, ch, 4), contiguous=True)
        if not rows:
            if out is not None:
                raise ValueError("rows=False writes no rows: pass no `out`")
        elif out is None:
            out = torch.empty((n, ch, frames), dtype=dtype, device=windows.device)
        else:
            e.tensor("out", out, dtype, run_extent("window_rows", rows=n, channels=ch, frames=frames), shape=(n, ch, frames),
                     contiguous=True)
        kind = kinds[dtype]
        cur = self.engine._enter() if ordered else None
        if placed and rows:
            _check("AADHip_WindowDecodePlanRunPlaced",
                   self.engine.lib.AADHip_WindowDecodePlanRunPlaced(self.handle, data.data_ptr(), n, windows.data_ptr(), spans.data_ptr(),
                                                                    frames, kind, out.data_ptr(),
                                                                    gain.data_ptr() if gain is not None else None,
                                                                    WINDOW_GAIN_ADD if accumulate else WINDOW_GAIN_STORE))
        elif placed:
            _check("AADHip_WindowDecodePlanRunPlacedStats",
                   self.engine.lib.AADHip_WindowDecodePlanRunPlacedStats(self.handle, data.data_ptr(), n, windows.data_ptr(),
                                                                         spans.data_ptr(), frames, stats.data_ptr()))
        elif gained:
            _check("AADHip_WindowDecodePlanRunGain",
                   self.engine.lib.AADHip_WindowDecodePlanRunGain(self.handle, data.data_ptr(), n, windows.data_ptr(), frames, kind,
                                                                  out.data_ptr(), gain.data_ptr() if gain is not None else None,
                                                                  WINDOW_GAIN_ADD if accumulate else WINDOW_GAIN_STORE))
        elif stats is None:
            _check("AADHip_WindowDecodePlanRun",
                   self.engine.lib.AADHip_WindowDecodePlanRun(self.handle, data.data_ptr(), n, windows.data_ptr(), frames, kind,
                                                              out.data_ptr()))
        else:
            _check("AADHip_WindowDecodePlanRunStats",
                   self.engine.lib.AADHip_WindowDecodePlanRunStats(self.handle, data.data_ptr(), n, windows.data_ptr(), frames, kind,
                                                                   out.data_ptr() if rows else None, stats.data_ptr()))
        if ordered:
            self.engine._exit(cur)
        if stats is None:
            return out
        return (out, stats) if rows else stats

    def close(self):
        if self.handle:
            self.engine.lib.AADHip_WindowDecodePlanDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fir_sample_type(torch, what, dtype):
    """the row type of a FIR stage (`what`: "resample", "convolve") -> (dtype, None: torch.float32; its AAD_HIP_SAMPLE_* value)"""
    dtype = torch.float32 if dtype is None else dtype
    kinds = {torch.float32: SAMPLE_FLOAT32, torch.int16: SAMPLE_INT16, torch.float16: SAMPLE_FLOAT16, torch.bfloat16: SAMPLE_BFLOAT16}
    if dtype not in kinds:
        raise ValueError("%s writes torch.float32, torch.int16, torch.float16 or torch.bfloat16, not %s" % (what, dtype))
    return dtype, kinds[dtype]


def _check_fir_run(e, what, n, device, channels, frames, dtype, out, gain, accumulate, spans, stats, rows):
    """every rule of the arguments of a FIR stage's run (Resampler.run, Convolver.run) for n windows on `device`, before any
    library call -> (channels, sample type, out, gain, accumulate, spans, stats or None)"""
    torch = e.torch
    dtype, kind = _fir_sample_type(torch, what, dtype)
    gained = gain is not None or bool(accumulate)
    placed = spans is not None
    with_stats = not (stats is None or stats is False)
    if placed:
        if with_stats and rows:
            raise ValueError("spans: no run with both rows and statistics - take the levels from a statistics-only run "
                             "(stats=True, rows=False, spans=...), then the rows")
        if rows and dtype == torch.int16:
            raise ValueError("spans: float rows only (torch.float32, torch.float16, torch.bfloat16), not torch.int16")
    n, ch, frames = int(n), int(channels), int(frames)
    if placed:
        spans = e.window_table(spans, True, name="spans", rows=n)
    if gained:
        if dtype == torch.int16:
            raise ValueError("gain / accumulate: float rows only (torch.float32, torch.float16, torch.bfloat16), not torch.int16")
        if with_stats or not rows:
            raise ValueError("gain / accumulate: no statistics variant - take the levels first from a statistics-only run "
                             "(stats=True, rows=False), then run with the gains")
        if accumulate and out is None:
            raise ValueError("accumulate=True adds into `out`: pass the rows to add to")
        if gain is not None:
            e.tensor("gain", gain, torch.float32, n, shape=(n,), contiguous=True)
    if not with_stats:
        stats = None
        if not rows:
            raise ValueError("rows=False is a statistics-only run: pass stats=True or a table")
    elif stats is True:
        stats = torch.empty((n, ch, 4), dtype=torch.int64, device=device)
    else:
        e.tensor("stats", stats, torch.int64, run_extent("stats", rows=n, channels=ch), shape=(n, ch, 4), contiguous=True)
    if not rows:
        if out is not None:
            raise ValueError("rows=False writes no rows: pass no `out`")
    elif out is None:
        out = torch.empty((n, ch, frames), dtype=dtype, device=device)
    else:
        e.tensor("out", out, dtype, run_extent("window_rows", rows=n, channels=ch, frames=frames), shape=(n, ch, frames),
                 contiguous=True)
    return ch, kind, out, gain, bool(accumulate), spans, stats


FirSource = namedtuple("FirSource", "rows lanes source_frames stats", defaults=(None,))  # FirStage.decode_source -> run_source
ResampleSource = ConvolveSource = FirSource  # a record built by hand without statistics serves every run that asks for none

_UNSET = object()  # a keyword that the caller did not pass


class FirStage:
    """What Resampler and Convolver share: a FIR stage behind window decode plans, run in three steps - AADHip_<PREFIX>Resolve, the
    plan's own run into an int16 source batch, AADHip_<PREFIX>Run[Gain|Stats].  A stage states PREFIX; SELECTOR, the keyword of its
    per-window table (run's fifth argument); WHAT, its name in refusals; STATS, whether it has a statistics run (both have) - where
    not, stats= and rows= are unknown keywords; CHECKS_SOURCE, whether run_source itself refuses a short source row."""
    PREFIX = SELECTOR = WHAT = None
    STATS = CHECKS_SOURCE = False

    def source_frames(self, frames):
        """T_src: the frames of a source row that `frames` output frames read (AADHip_<PREFIX>SourceFrames)"""
        n = C.c_uint32()
        name = self.PREFIX + "SourceFrames"
        _check(name, getattr(self.engine.lib, name)(self.handle, int(frames), C.byref(n)))
        return n.value

    def _keywords(self, where, named, stats, rows, selector=_UNSET):
        """-> (selector, stats, rows) of a call: the selector in place or under the stage's keyword; any other keyword - of a stage
        without a statistics run stats= and rows= too - is refused as Python refuses an unknown one"""
        named = dict(named)
        if selector is not _UNSET:
            selector = named.pop(self.SELECTOR, selector)
        if not self.STATS:
            named.update((k, v) for k, v in (("stats", stats), ("rows", rows)) if v is not _UNSET)
        for k in named:
            raise TypeError("%s.%s() got an unexpected keyword argument '%s'" % (type(self).__name__, where, k))
        return selector, None if stats is _UNSET else stats, True if rows is _UNSET else rows

    @classmethod
    def check_run(cls, e, window_plan, windows, frames, selector, dtype, out, gain, accumulate, spans, stats, rows):
        """every rule of run's arguments on engine `e`, before any library call and without a stage -> (the window table,
        (channels, sample type, out, gain, accumulate, spans, stats or None))"""
        _fir_sample_type(e.torch, cls.WHAT, dtype)  # the order of the checks is the one the call had before it took gain, spans and stats
        windows = e.window_table(windows, True)
        n = int(windows.shape[0])
        if selector is not None:
            e.tensor(cls.SELECTOR, selector, e.torch.int64, n, shape=(n,), contiguous=True)
        return windows, _check_fir_run(e, cls.WHAT, n, windows.device, window_plan.header.num_channels, frames, dtype, out, gain,
                                       accumulate, spans, stats, rows)

    def run(self, window_plan, data, windows, frames, selector=None, dtype=None, out=None, gain=None, accumulate=False, spans=None,
            stats=_UNSET, rows=_UNSET, **named):
        """window_plan: a WindowDecodePlan of any kind over `data`; windows: int64 cuda tensor [N, 2] of (stream, first_frame in
        source frames); selector (variant= of a Resampler, response= of a Convolver): contiguous int64 cuda tensor [N], None for
        all 0 -> `out` ([N, channels, frames] of dtype torch.float32, torch.int16, torch.float16 or torch.bfloat16; allocated when
        None): window w through the filter its selector names - the ratio select[stream][variant[w]], the response response[w] -
        zeros where there is none.  Three steps on the engine's stream, ordered against torch's current one: the stage's Resolve,
        the plan's own run into an int16 source batch of source_frames(frames) frames per row, and the stage's Run.  Neither table
        is read on the host.  The source batch and the tables between the steps are temporaries of this call; torch's current
        stream waits for the engine's before it can reuse them (Engine.window_table).
        gain, accumulate, spans, stats, rows: the meanings and refusals of WindowDecodePlan.run, on the filtered rows - `spans`
        in OUTPUT frames; the FIR step is then the stage's RunGain or RunStats, and with stats the source batch is decoded with
        its own statistics, whose `count` the FIR turns into the row's -> out, (out, stats) or stats.  The statistics are those
        of the int16 row: a float row past full scale keeps its value, its record is clamped (max_abs 32767 or 32768 is the
        witness).  The call is decode_source and run_source composed."""
        selector, stats, rows = self._keywords("run", named, stats, rows, selector)
        windows, checked = self.check_run(self.engine, window_plan, windows, frames, selector, dtype, out, gain, accumulate, spans, stats,
                                          rows)
        source = self.decode_source(window_plan, data, windows, frames, selector, checked[-1] is not None if self.STATS else _UNSET)
        return self._run_source(source, frames, *checked)

    def decode_source(self, window_plan, data, windows, frames, selector=None, stats=_UNSET, **named):
        """The first two steps of run: the stage's Resolve and the plan's own run into the int16 source batch, with stats=True by
        AADHip_WindowDecodePlanRunStats -> FirSource(rows int16 [N, channels, source_frames], lanes int32 [N, 2],
        source_frames, stats int64 [N, channels, 4] or None), what run_source reads - several times for one decode, as
        Engine.mix_windows_resampled and Engine.mix_windows_reverberated do."""
        selector, stats, _ = self._keywords("decode_source", named, stats, _UNSET, selector)
        e = self.engine
        torch = e.torch
        windows = e.window_table(windows, True)
        n, frames = int(windows.shape[0]), int(frames)
        if selector is not None:
            e.tensor(self.SELECTOR, selector, torch.int64, n, shape=(n,), contiguous=True)
        source_frames = self.source_frames(frames)
        source_windows = torch.empty((n, 2), dtype=torch.int64, device=windows.device)
        lanes = torch.empty((n, 2), dtype=torch.int32, device=windows.device)
        cur = e._enter()
        _check(self.PREFIX + "Resolve",
               getattr(e.lib, self.PREFIX + "Resolve")(self.handle, n, windows.data_ptr(), selector.data_ptr() if selector is not None else None,
                                                      frames, source_windows.data_ptr(), lanes.data_ptr()))
        if stats:
            rows, table = window_plan.run(data, source_windows, source_frames, torch.int16, ordered=False, stats=True)
        else:
            rows, table = window_plan.run(data, source_windows, source_frames, torch.int16, ordered=False), None
        e._exit(cur)
        return FirSource(rows, lanes, source_frames, table)

    def run_source(self, source, frames, channels, dtype=None, out=None, gain=None, accumulate=False, spans=None, stats=_UNSET,
                   rows=_UNSET, **named):
        """The FIR step alone: the stage's Run, with gain / accumulate / spans its RunGain, with stats its RunStats (the source must
        have been decoded with stats=True) - over decode_source's record or, for a Convolver, any int16 rows [N,
        channels, source_frames] with a lane table int32 [N, 2] of (response, shift): the rows of Resampler.run(dtype=torch.int16)
        with a table of the caller's, for one.  channels: the rows per window of the plan that decoded the source - the record is
        held to it: rows [N, channels, source_frames], statistics [N, channels, 4], lanes [N, 2], contiguous, refused otherwise
        before any library call.  Arguments and return values as run."""
        _, stats, rows = self._keywords("run_source", named, stats, rows)
        e = self.engine
        torch = e.torch
        _fir_sample_type(torch, self.WHAT, dtype)
        # the C calls take the record's pointers and `channels` rows per window: the record must be of that many
        e.tensor("source.lanes", source.lanes, torch.int32, shape=(None, 2), contiguous=True)
        n, ch, t_src = int(source.lanes.shape[0]), int(channels), int(source.source_frames)
        e.tensor("source.rows", source.rows, torch.int16, run_extent("window_rows", rows=n, channels=ch, frames=t_src),
                 shape=(n, ch, t_src), contiguous=True)
        if self.STATS and source.stats is not None:
            e.tensor("source.stats", source.stats, torch.int64, run_extent("stats", rows=n, channels=ch), shape=(n, ch, 4), contiguous=True)
        checked = _check_fir_run(e, self.WHAT, n, source.lanes.device, ch, frames, dtype, out, gain, accumulate, spans, stats, rows)
        if checked[-1] is not None and source.stats is None:
            raise ValueError("stats: the source batch carries no statistics - decode it with decode_source(..., stats=True)")
        if self.CHECKS_SOURCE and int(frames) > 0 and t_src < self.source_frames(frames):
            raise ValueError("source.rows: %d frames per row where %d output frames read %d" % (t_src, int(frames), self.source_frames(frames)))
        return self._run_source(source, frames, *checked)

    def _run_source(self, source, frames, ch, kind, out, gain, accumulate, spans, stats):
        e = self.engine
        n, frames = int(source.lanes.shape[0]), int(frames)
        head = (self.handle, n, ch, source.rows.data_ptr(), source.source_frames, source.lanes.data_ptr())
        spans_ptr = spans.data_ptr() if spans is not None else None
        if stats is not None:
            name, tail = "RunStats", (source.stats.data_ptr(), spans_ptr, frames, kind, out.data_ptr() if out is not None else None,
                                      stats.data_ptr())
        elif gain is not None or accumulate or spans is not None:
            name, tail = "RunGain", (spans_ptr, frames, kind, out.data_ptr(), gain.data_ptr() if gain is not None else None,
                                     WINDOW_GAIN_ADD if accumulate else WINDOW_GAIN_STORE)
        else:
            name, tail = "Run", (frames, kind, out.data_ptr())
        cur = e._enter()
        _check(self.PREFIX + name, getattr(e.lib, self.PREFIX + name)(*head, *tail))
        e._exit(cur)
        if stats is None:
            return out
        return (out, stats) if out is not None else stats

    def close(self):
        if self.handle:
            getattr(self.engine.lib, self.PREFIX + "Destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Resampler(FirStage):
    """AADHip_Resampler*: banks of integer polyphase filters and the table that picks one per (stream, variant)."""
    PREFIX, SELECTOR, WHAT, STATS = "AADHip_Resampler", "variant", "resample", True

    def __init__(self, engine, handle, ratios, select):
        self.engine, self.handle, self.ratios, self.select = engine, handle, ratios, select

    def bank(self, r):
        """-> (L, M, int16 array [L, K]): ratio r reduced, and its bank - phase p's K taps in Q14 (AADHip_ResamplerBank)"""
        lib = self.engine.lib
        L, M, K = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check("AADHip_ResamplerBank", lib.AADHip_ResamplerBank(self.handle, int(r), C.byref(L), C.byref(M), C.byref(K), None, 0))
        h = np.zeros((L.value, K.value), dtype=np.int16)
        _check("AADHip_ResamplerBank", lib.AADHip_ResamplerBank(self.handle, int(r), C.byref(L), C.byref(M), C.byref(K), h.ctypes.data, h.size))
        return L.value, M.value, h


class Convolver(FirStage):
    """AADHip_Convolver*: impulse responses as int16 taps with a scale exponent and a delay, one picked per window; T_src = frames +
    the longest response's taps - 1."""
    PREFIX, SELECTOR, WHAT, STATS, CHECKS_SOURCE = "AADHip_Convolver", "response", "convolve", True, True

    def __init__(self, engine, handle, num_responses):
        self.engine, self.handle, self.num_responses = engine, handle, num_responses

    def response(self, r):
        """-> (q, delay, int16 array [K]): response r as the library quantised it - h_q = rint(h * 2^q) (AADHip_ConvolverResponse)"""
        lib = self.engine.lib
        K, q, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check("AADHip_ConvolverResponse", lib.AADHip_ConvolverResponse(self.handle, int(r), C.byref(K), C.byref(q), C.byref(d), None, 0))
        h = np.zeros(K.value, dtype=np.int16)
        _check("AADHip_ConvolverResponse",
               lib.AADHip_ConvolverResponse(self.handle, int(r), C.byref(K), C.byref(q), C.byref(d), h.ctypes.data, h.size))
        return q.value, d.value, h


def _spectrogram_arguments(n_fft, hop, win_length, window, filters):
    """what `spectrogram` refuses, before anything is built -> (n_fft, hop, win_length, float32 window, float32 filters or None)"""
    n_fft, hop = int(n_fft), int(hop)
    win_length = n_fft if win_length is None else int(win_length)
    if not (1 <= win_length <= n_fft <= 4096) or not (1 <= hop < 1 << 32):
        raise ValueError("n_fft, win_length, hop: 1 <= win_length <= n_fft <= 4096 and hop >= 1 are needed, got %d, %d, %d"
                         % (n_fft, win_length, hop))
    if window is None:
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length, dtype=np.float64) / win_length)
    window = np.ascontiguousarray(np.asarray(window, dtype=np.float64).reshape(-1).astype(np.float32))
    if window.size != win_length or not np.isfinite(window).all():
        raise ValueError("window: %d finite values are needed, got %d values" % (win_length, window.size))
    if filters is not None:
        filters = np.ascontiguousarray(np.asarray(filters, dtype=np.float32))
        bins = n_fft // 2 + 1
        if filters.ndim != 2 or filters.shape[0] == 0 or filters.shape[1] != bins:
            raise ValueError("filters: shape [M >= 1, %d] is needed, got %s" % (bins, filters.shape))
        a = np.abs(filters)
        if not np.isfinite(filters).all() or bool(((a != 0) & (a < 2.0 ** -60)).any()):
            raise ValueError("filters: every weight finite, every nonzero weight at least 2^-60 in magnitude")
    return n_fft, hop, win_length, window, filters


def mel_filters(rate, n_fft, n_mels, f_min=0.0, f_max=None):
    """HTK triangular mel filters, unnormalised -> float32 numpy array [n_mels, n_fft // 2 + 1], computed in float64:
    mel(f) = 2595 log10(1 + f / 700); n_mels + 2 points evenly spaced in mel from f_min to f_max (None: rate / 2); filter j rises
    from point j to point j + 1 and falls to point j + 2 over the bin frequencies k rate / n_fft:
    max(0, min((f - p[j]) / (p[j + 1] - p[j]), (p[j + 2] - f) / (p[j + 2] - p[j + 1]))).  A weight that rounds below 2^-60 is 0."""
    rate, n_fft, n_mels = float(rate), int(n_fft), int(n_mels)
    f_max = rate / 2.0 if f_max is None else float(f_max)
    if n_mels < 1 or n_fft < 1 or not (0.0 <= float(f_min) < f_max):
        raise ValueError("mel_filters: n_mels >= 1, n_fft >= 1 and 0 <= f_min < f_max are needed")
    lo, hi = (2595.0 * np.log10(1.0 + f / 700.0) for f in (float(f_min), f_max))
    points = 700.0 * (10.0 ** (np.linspace(lo, hi, n_mels + 2) / 2595.0) - 1.0)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * rate / n_fft
    rise = (f[None, :] - points[:-2, None]) / (points[1:-1] - points[:-2])[:, None]
    fall = (points[2:, None] - f[None, :]) / (points[2:] - points[1:-1])[:, None]
    w = np.maximum(0.0, np.minimum(rise, fall)).astype(np.float32)
    w[np.abs(w) < 2.0 ** -60] = 0
    return w


def frame_counts(count, win_length, hop):
    """The padding mask of the features: for the `count` column of any statistics table (the leading frames of a row that the
    stream had), the frames of the row's spectrogram that lie wholly inside the stream: 0 for count < win_length, else
    1 + (count - win_length) // hop.  count: a torch tensor, a numpy array or an int -> the same kind."""
    w, h = int(win_length), int(hop)
    if w < 1 or h < 1:
        raise ValueError("frame_counts: win_length >= 1 and hop >= 1 are needed")
    if hasattr(count, "clamp"):  # torch
        return ((count - w).div(h, rounding_mode="floor") + 1).clamp(min=0)
    return np.maximum((np.asarray(count, dtype=np.int64) - w) // h + 1, 0)


class Spectrogram:
    """AADHip_Spectrogram*: a framed, windowed real DFT with int16 coefficients and, with filters, the filterbank behind it."""

    def __init__(self, engine, handle, n_fft, hop, win_length, num_filters):
        self.engine, self.handle, self.n_fft, self.hop, self.win_length, self.num_filters = engine, handle, n_fft, hop, win_length, num_filters
        self.bins = n_fft // 2 + 1
        self.columns = num_filters if num_filters else self.bins  # the last dimension of run's result

    def frames(self, T):
        """F = 1 + (T - win_length) // hop of rows of T elements (AADHip_SpectrogramFrames)"""
        n = C.c_uint32()
        _check("AADHip_SpectrogramFrames", self.engine.lib.AADHip_SpectrogramFrames(self.handle, int(T), C.byref(n)))
        return n.value

    def coefficients(self):
        """-> (q, int16 array [win_length, bins, 2]): the cos and -sin matrices as the library quantised them"""
        lib = self.engine.lib
        q = C.c_uint32()
        m = np.zeros((self.win_length, self.bins, 2), dtype=np.int16)
        _check("AADHip_SpectrogramCoefficients", lib.AADHip_SpectrogramCoefficients(self.handle, C.byref(q), m.ctypes.data, m.size))
        return q.value, m

    def _rows(self, name, rows):
        """an int16 row batch [N, C, T] or [R, T] that a run reads where it lies -> (leading shape, T, rows, pitch)"""
        e = self.engine
        torch = e.torch
        e.tensor(name, rows, torch.int16)
        if rows.dim() not in (2, 3):
            raise ValueError("%s: [N, C, T] or [R, T] is needed, got shape %s" % (name, tuple(rows.shape)))
        lead, T = [int(v) for v in rows.shape[:-1]], int(rows.shape[-1])
        if T < self.win_length:
            raise ValueError("%s: %d elements a row, below the window's %d - such a row has no frame" % (name, T, self.win_length))
        n = int(np.prod(lead))
        # one pitch: the stride of the innermost leading dimension with more than one row, the outer ones its multiples
        strides = [int(v) for v in rows.stride()[:-1]]
        pitch, step = T, None
        for size, stride in zip(reversed(lead), reversed(strides)):
            if size > 1:
                if step is None:
                    pitch = step = stride
                elif stride != step:
                    raise ValueError("%s: one pitch between consecutive rows is needed, got shape %s with strides %s - pass "
                                     "%s.contiguous() if a copy is intended" % (name, tuple(rows.shape), tuple(rows.stride()), name))
            step = None if step is None else step * size
        if pitch < T:
            raise ValueError("%s: a row pitch of at least %d elements is needed, got strides %s" % (name, T, tuple(rows.stride())))
        e.tensor(name, rows, torch.int16, (n - 1) * pitch + T if n else 0, rows_in_place=True)
        return lead, T, n, pitch

    def _out(self, rows, lead, T, n, out):
        """the result of a run over `rows`: float32 [lead.., F, columns], the caller's when it fits"""
        torch = self.engine.torch
        F = 1 + (T - self.win_length) // self.hop
        shape = tuple(lead) + (F, self.columns)
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=rows.device)
        return self.engine.tensor("out", out, torch.float32, n * F * self.columns, shape=shape, contiguous=True)

    def run(self, rows, out=None):
        """rows: int16 cuda tensor [N, C, T] or [R, T], read where it lies: stride(-1) == 1 and one pitch between consecutive
        rows, at least T - a window decode's, Resampler.run's or Convolver.run's rows with dtype=torch.int16, or a slice of them
        -> out float32 [N, C, F, columns] or [R, F, columns], contiguous, allocated when None.  Asynchronous on the engine's
        stream, ordered against torch's current one."""
        e = self.engine
        lead, T, n, pitch = self._rows("rows", rows)
        out = self._out(rows, lead, T, n, out)
        if n == 0:
            return out
        cur = e._enter()
        _check("AADHip_SpectrogramRun", e.lib.AADHip_SpectrogramRun(self.handle, n, rows.data_ptr(), pitch, T, out.data_ptr()))
        e._exit(cur)
        return out

    def run_mix(self, rows, other, gain=None, other_gain=None, spans=None, out=None):
        """The spectrogram of gain * rows + other_gain * other, summed and quantised to int16 while the kernel stages its samples
        (AADHip_SpectrogramRunMix, include/aad_hip.h "spectrogram", paragraph "mix"): per element
        clamp(rint(fl32(fl32(gain * rows) + fl32(other_gain * other)))), ties to even, a NaN 0 - no float32 batch, no quantise
        pass.  rows, other: int16 cuda tensors of one shape [N, C, T] or [R, T], each read where it lies under `run`'s one-pitch
        rule, each with a pitch of its own.  gain, other_gain: float32 cuda [N] - one pair for the C rows of a window - or [R],
        None for 1.  spans: int64 cuda [N, 2] or [R, 2] of (num_frames, out_frame): `other` is an event of num_frames elements
        added from element out_frame of the row on, clipped to the row as WindowDecodePlan.run clips a span; None for the whole
        row.  -> out as `run`."""
        e = self.engine
        torch = e.torch
        lead, T, n, pitch = self._rows("rows", rows)
        if torch.is_tensor(other) and tuple(other.shape) != tuple(rows.shape):
            raise ValueError("other: shape %s, that of rows, is needed, got %s" % (tuple(rows.shape), tuple(other.shape)))
        other_pitch = self._rows("other", other)[3]
        groups, per = lead[0], n // lead[0] if lead[0] else 1
        for name, g in (("gain", gain), ("other_gain", other_gain)):
            if g is not None:
                e.tensor(name, g, torch.float32, groups, shape=(groups,), contiguous=True)
        if spans is not None:
            e.tensor("spans", spans, torch.int64, 2 * groups, shape=(groups, 2), contiguous=True)
        out = self._out(rows, lead, T, n, out)
        if n == 0:
            return out
        ptr = lambda t: None if t is None else t.data_ptr()
        cur = e._enter()
        _check("AADHip_SpectrogramRunMix",
               e.lib.AADHip_SpectrogramRunMix(self.handle, n, rows.data_ptr(), pitch, other.data_ptr(), other_pitch, per, ptr(gain),
                                              ptr(other_gain), ptr(spans), T, out.data_ptr()))
        e._exit(cur)
        return out

    def close(self):
        if self.handle:
            self.engine.lib.AADHip_SpectrogramDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipEvent:
    """A hipEvent_t of our own (timing disabled): what AADHip_ContextSignalNextRun takes and hipStreamWaitEvent waits for.
    torch.cuda.Event cannot wrap a foreign handle and creates its own lazily, hence the few runtime calls made directly."""
    _hip = None

    @classmethod
    def runtime(cls):
        if cls._hip is None:
            # THE runtime this process already runs on (torch's / libaad_hip.so's): a second copy would not know our streams
            path = "libamdhip64.so"
            try:
                with open("/proc/self/maps") as maps:
                    for line in maps:
                        if "libamdhip64.so" in line:
                            path = line.split()[-1]
                            break
            except OSError:
                pass
            hip = C.CDLL(path)
            hip.hipEventCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
            hip.hipEventDestroy.argtypes = [C.c_void_p]
            hip.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
            hip.hipEventSynchronize.argtypes = [C.c_void_p]
            hip.hipEventQuery.argtypes = [C.c_void_p]
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            cls._hip = hip
        return cls._hip

    def __init__(self, timing=False):
        self.handle = C.c_void_p()
        rc = self.runtime().hipEventCreateWithFlags(C.byref(self.handle), 0x0 if timing else 0x2)  # hipEventDisableTiming
        if rc != 0:
            raise RuntimeError("hipEventCreateWithFlags failed (%d)" % rc)

    def wait_on(self, stream):
        """stream: a torch.cuda.Stream - everything queued on it afterwards waits for this event"""
        rc = self.runtime().hipStreamWaitEvent(C.c_void_p(stream.cuda_stream), self.handle, 0)
        if rc != 0:
            raise RuntimeError("hipStreamWaitEvent failed (%d)" % rc)

    def elapsed_ms(self, stop):
        """milliseconds from this (start) event to `stop`, both created with timing=True and both complete"""
        ms = C.c_float()
        rc = self.runtime().hipEventElapsedTime(C.byref(ms), self.handle, stop.handle)
        if rc != 0:
            raise RuntimeError("hipEventElapsedTime failed (%d)" % rc)
        return float(ms.value)

    def synchronize(self):
        rc = self.runtime().hipEventSynchronize(self.handle)
        if rc != 0:
            raise RuntimeError("hipEventSynchronize failed (%d)" % rc)

    def close(self):
        if self.handle:
            self.runtime().hipEventDestroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# whether an EncodeDecodePipeline gives its engines SIMD roles by default (DESIGN.md "SIMD roles")
PIPELINE_SIMD_ROLES = True


class SimdRoleAllocator:
    """Free-slot allocator of the SIMD roles of one device's pipelines.  A pipeline takes one slot = (encoder SIMD, decoder SIMD);
    the two slots are (0, 1) and (2, 3), so that the four engines of two live pipelines hold four different SIMDs and the two
    encoders sit on different halves of the CU's LDS path ({0, 1} and {2, 3}).  A third live pipeline gets None: no roles.
    The roles are IN FORCE only while both slots are taken: a pipeline that runs alone keeps today's launches - its two kernels
    cannot share a CU then (their LDS does not fit), let alone a SIMD, and under roles they would (measured: one pipeline alone
    2.5 % slower with roles, DESIGN.md "SIMD roles").  `apply` of every holder is called whenever that changes."""
    SLOTS = ((0, 1), (2, 3))

    def __init__(self):
        self.taken = [False] * len(self.SLOTS)
        self.holders = [None] * len(self.SLOTS)  # per slot: apply(encoder SIMD or None, decoder SIMD or None)

    def in_force(self):
        return all(self.taken)

    def acquire(self, apply=None):
        """-> slot index, or None when every slot is taken.  apply(enc_simd, dec_simd): sets the holder's roles"""
        for i, t in enumerate(self.taken):
            if not t:
                self.taken[i] = True
                self.holders[i] = apply
                self._apply_all()
                return i
        return None

    def release(self, slot):
        if slot is not None and self.taken[slot]:
            apply = self.holders[slot]
            self.taken[slot], self.holders[slot] = False, None
            if apply is not None:
                apply(None, None)
            self._apply_all()

    def roles(self, slot):
        """-> (encoder SIMD, decoder SIMD) of a slot while the roles are in force, else (None, None)"""
        return self.SLOTS[slot] if slot is not None and self.taken[slot] and self.in_force() else (None, None)

    def _apply_all(self):
        for i, apply in enumerate(self.holders):
            if self.taken[i] and apply is not None:
                apply(*self.roles(i))


_simd_roles = {}  # device index -> SimdRoleAllocator


class EncodeDecodePipeline:
    """Encode on one context, decode on another: the encode of step k+1 runs while step k decodes.

    On a batch that fills only part of the chip (BASELINE's 1000 one-block streams occupy 125 of 256
    CUs with either kernel) the two kernels of consecutive steps share the device instead of taking
    turns.  Two streams ordered by events; the .aad images go through a ring of buffers so that an
    encode never overwrites what a decode still reads (one wait per half ring: the decode stream runs
    in order).  The "encoded" events ride on the encode kernels' own dispatch packets (Engine.signal_next): an
    event recorded BEHIND every encode costs the encode queue 3 us per step (tools/experiments/launch_gap_probe.py).
    Every step encodes its whole batch and decodes exactly what it encoded; `pcm` and `out`
    are the caller's and must stay untouched until the step's kernels have run."""

    def __init__(self, enc_engine, dec_engine, param, streams, samples, ring=8, simd_roles=PIPELINE_SIMD_ROLES):
        assert ring >= 2 and ring % 2 == 0
        assert enc_engine.stream.cuda_stream != dec_engine.stream.cuda_stream, "the two contexts need streams of their own"
        torch = enc_engine.torch
        self.torch, self.ring, self.k = torch, ring, 0
        self.enc_engine, self.dec_engine = enc_engine, dec_engine
        # Two pipelines that are alive together run their kernels side by side: each gives its two engines SIMDs of their own
        # (SimdRoleAllocator), so that the one busy wave of every such kernel finds a SIMD no other kernel's busy wave uses.
        self._take_simd_roles(_simd_roles.setdefault(enc_engine.device, SimdRoleAllocator()) if simd_roles else None)
        self.enc = enc_engine.uniform_encode_plan(param, streams, samples)
        self.images = [torch.zeros((streams, self.enc.stride), dtype=torch.uint8, device="cuda:%d" % enc_engine.device)
                       for _ in range(ring)]
        # the header comes from a first encode of silence: the decode plan needs the block geometry
        zero = torch.zeros((streams, samples, param.num_channels), dtype=torch.int16, device=self.images[0].device)
        self.enc.run(zero, self.images[0])
        torch.cuda.synchronize()
        self.header = parse_header(bytes(self.images[0][0, :31].cpu().numpy()))
        self.dec = dec_engine.uniform_decode_plan(self.header, streams, self.images[0].stride(0), self.enc.image_size)
        self.encoded = [HipEvent() for _ in range(ring)]
        self.decoded = [torch.cuda.Event() for _ in range(ring)]

    def step(self, pcm, out, timing=None):
        """timing: four HipEvent(timing=True) -> start / end of the encode kernel, start / end of the decode kernel, carried by
        the kernels' own dispatches like the ordering events (elapsed_ms between a pair = the kernel's own duration)"""
        k, ring = self.k, self.ring
        self.k += 1
        b = k % ring
        s_enc, s_dec = self.enc_engine.stream, self.dec_engine.stream
        if k >= ring and k % (ring // 2) == 0:  # covers the half ring of encodes that follows
            s_enc.wait_event(self.decoded[(k - ring // 2 - 1) % ring])
        encoded = self.encoded[b] if timing is None else timing[1]
        self.enc_engine.signal_next(encoded, start=None if timing is None else timing[0])
        self.enc.run(pcm, self.images[b], None, ordered=False)
        encoded.wait_on(s_dec)
        if timing is not None:
            self.dec_engine.signal_next(timing[3], start=timing[2])
        self.dec.run(self.images[b], out, ordered=False)
        self.decoded[b].record(s_dec)
        return self.images[b]

    def close(self):
        self.torch.cuda.synchronize()
        self.enc.close()
        self.dec.close()
        for e in self.encoded:
            e.close()
        self._release_simd_roles()

    def _take_simd_roles(self, allocator):
        """allocator: the device's SimdRoleAllocator, None: no roles"""
        self._roles = allocator
        self._role_slot = allocator.acquire(self._set_simd_roles) if allocator is not None else None

    def _set_simd_roles(self, enc_simd, dec_simd):
        self.enc_engine.set_simd_role(enc_simd)
        self.dec_engine.set_simd_role(dec_simd)

    def _release_simd_roles(self):
        if getattr(self, "_role_slot", None) is not None:
            self._roles.release(self._role_slot)
            self._role_slot = None


def parse_header(data):
    """31-byte big-endian file header (reference src/aad_decoder.c:99-170) -> AADHeaderInfo"""
    if len(data) < 31 or data[:4] != b"AAD\x00":
        raise ApiError("parse_header", AADApiResult.INVALID_FORMAT)
    be = lambda o, n: int.from_bytes(data[o:o + n], "big")
    return AADHeaderInfo(format_version=be(4, 4), codec_version=be(8, 4), num_channels=be(12, 2),
                         num_samples=be(14, 4), sampling_rate=be(18, 4), bits_per_sample=be(22, 2),
                         block_size=be(24, 2), num_samples_per_block=be(26, 4), ch_process_method=data[30])


__all__ = ["Engine", "EncodePlan", "PlanarEncodePlan", "PlanarReconstructPlan", "DecodePlan", "WindowDecodePlan", "FirStage", "Resampler", "Convolver", "Spectrogram", "mel_filters", "frame_counts", "EncodeDecodePipeline", "SimdRoleAllocator", "parse_header", "make_parameter", "LANE_STATE_DTYPE", "rmse", "snr_db", "level_dbfs", "snr_gains", "select_least_bits", "run_extent", "tensor_span"]
