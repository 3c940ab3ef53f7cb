"""ctypes view of the C-ABI in include/*.h.

``LegacyCodec`` drives the reference-shaped API (AADEncoder_* / AADDecoder_*, reference
src/aad_encoder.h:25-50, src/aad_decoder.h:15-42) of ANY library exporting it: this repo's
libaad_hip.so in production, the compiled reference (oracle/_ref/libaadref.so) in the tests -
the same call sequence the reference CLI uses (src/main.c:91-106, 182-198).
"""
import ctypes as C
import os

import numpy as np


class AADApiResult:
    OK = 0
    INVALID_ARGUMENT = 1
    INVALID_FORMAT = 2
    INSUFFICIENT_BUFFER = 3
    INSUFFICIENT_DATA = 4
    PARAMETER_NOT_SET = 5
    NG = 6
    _names = {0: "OK", 1: "INVALID_ARGUMENT", 2: "INVALID_FORMAT", 3: "INSUFFICIENT_BUFFER",
              4: "INSUFFICIENT_DATA", 5: "PARAMETER_NOT_SET", 6: "NG"}

    @classmethod
    def name(cls, v):
        return cls._names.get(int(v), str(v))


class AADHeaderInfo(C.Structure):  # include/aad.h
    _fields_ = [("format_version", C.c_uint32), ("codec_version", C.c_uint32),
                ("num_channels", C.c_uint16), ("num_samples", C.c_uint32),
                ("sampling_rate", C.c_uint32), ("bits_per_sample", C.c_uint16),
                ("block_size", C.c_uint16), ("num_samples_per_block", C.c_uint32),
                ("ch_process_method", C.c_int)]


class AADEncodeParameter(C.Structure):  # include/aad_encoder.h
    _fields_ = [("num_channels", C.c_uint16), ("sampling_rate", C.c_uint32),
                ("bits_per_sample", C.c_uint16), ("max_block_size", C.c_uint16),
                ("ch_process_method", C.c_int), ("num_encode_trials", C.c_uint8)]


class AADHipStreamDesc(C.Structure):  # include/aad_hip.h
    _fields_ = [("pcm_offset", C.c_uint64), ("data_offset", C.c_uint64),
                ("data_size", C.c_uint64), ("num_samples", C.c_uint32), ("reserved", C.c_uint32)]


class AADHipSegmentation(C.Structure):  # include/aad_hip.h
    _fields_ = [("segment_blocks", C.c_uint32), ("warmup_blocks", C.c_uint32)]


class AADHipPlanarLayout(C.Structure):  # include/aad_hip.h
    _fields_ = [("sample_type", C.c_int32), ("reserved", C.c_uint32), ("channel_stride", C.c_uint64)]


class AADHipPlanarOutput(C.Structure):  # include/aad_hip.h
    _fields_ = [("sample_type", C.c_int32), ("reserved", C.c_uint32), ("stream_stride", C.c_uint64), ("channel_stride", C.c_uint64)]


class AADHipRowStats(C.Structure):  # include/aad_hip.h: one row of a torch int64 [N, C, 4] tensor
    _fields_ = [("sum_sq", C.c_uint64), ("sum_abs", C.c_uint64), ("max_abs", C.c_uint64), ("count", C.c_uint64)]


class AADHipWindowSpan(C.Structure):  # include/aad_hip.h: one row of a torch int64 [N, 2] tensor (WindowDecodePlan.run with spans)
    _fields_ = [("num_frames", C.c_uint64), ("out_frame", C.c_uint64)]


class AADHipResampleRatio(C.Structure):  # include/aad_hip.h: output rate / source rate
    _fields_ = [("up", C.c_uint32), ("down", C.c_uint32)]


class AADHipResampleLane(C.Structure):  # include/aad_hip.h: one row of a torch int32 [N, 2] tensor (Resampler.run)
    _fields_ = [("bank", C.c_uint32), ("shift", C.c_uint32)]


class AADHipConvolveLane(C.Structure):  # include/aad_hip.h: one row of a torch int32 [N, 2] tensor (Convolver.run)
    _fields_ = [("response", C.c_uint32), ("shift", C.c_uint32)]


class AADHipLaneState(C.Structure):  # include/aad_hip.h
    _fields_ = [("weight", C.c_int32 * 4), ("history", C.c_int32 * 4),
                ("stepsize_index", C.c_int32), ("quantize_error", C.c_int32)]


STREAM_DESC_DTYPE = np.dtype([("pcm_offset", "<u8"), ("data_offset", "<u8"), ("data_size", "<u8"),
                              ("num_samples", "<u4"), ("reserved", "<u4")])
ERROR_STATS_DTYPE = np.dtype([("rms_error", "<f8"), ("mean_abs_error", "<f8"), ("max_abs_error", "<f8")])  # AADHipErrorStats
WINDOW_DTYPE = np.dtype([("stream", "<i8"), ("first_frame", "<i8")])  # struct AADHipWindow: an int64 pair, a torch int64 [N, 2] row
SAMPLE_INT16, SAMPLE_FLOAT32 = 0, 1  # enum AADHipSampleType
SAMPLE_FLOAT16, SAMPLE_BFLOAT16 = 4, 5  # window decode rows alone (WindowDecodePlan.run)
RESAMPLE_NO_BANK = 0xFFFF  # a select entry of AADHip_ResamplerCreate: the row is zeros
WINDOW_GAIN_STORE, WINDOW_GAIN_ADD = 0, 1  # enum AADHipWindowGainMode (WindowDecodePlan.run with gain / accumulate)
RECONSTRUCT_DECODED, RECONSTRUCT_RESIDUAL = 0, 1  # enum AADHipReconstructOutput
OPTION_LANE_MAPPING, OPTION_TRIAL_LANES, OPTION_STAGING_THREADS, OPTION_TILE_KBYTES, OPTION_COMPARE_ORDER = 0, 1, 2, 3, 4  # enum AADHipOption
LANE_MAPPINGS = {"auto": 0, "dense": 1, "quad": 2, "quad-fused": 3, "dense-tiled": 4}  # enum AADHipLaneMapping
TRIAL_LANES = {"dual": 0, "single": 1}  # enum AADHipTrialLanes
OPTION_SIMD_ROLE = 5  # enum AADHipOption; value: SIMD_ROLE_OFF or the SIMD (0..3) that runs the context's latency-bound waves
SIMD_ROLE_OFF = -1
LANE_STATE_DTYPE = np.dtype([("weight", "<i4", (4,)), ("history", "<i4", (4,)),
                             ("stepsize_index", "<i4"), ("quantize_error", "<i4")])

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIBRARY_PATH = os.environ.get("AAD_HIP_LIBRARY", os.path.join(_PKG_DIR, "libaad_hip.so"))

LEGACY_SYMBOLS = [
    "AADEncoder_CalculateBlockSize", "AADEncoder_EncodeHeader", "AADEncoder_CalculateWorkSize",
    "AADEncoder_Create", "AADEncoder_Destroy", "AADEncoder_SetEncodeParameter", "AADEncoder_EncodeWhole",
    "AADDecoder_DecodeHeader", "AADDecoder_CalculateWorkSize", "AADDecoder_Create", "AADDecoder_Destroy",
    "AADDecoder_SetHeader", "AADDecoder_DecodeBlock", "AADDecoder_DecodeWhole",
]
HIP_SYMBOLS = [
    "AADHip_GetDeviceCount", "AADHip_ContextCreate", "AADHip_ContextDestroy", "AADHip_ContextSynchronize",
    "AADHip_ContextLastError", "AADHip_ContextSignalNextRun", "AADHip_SignalNextRunSupported", "AADHip_ContextSetOption", "AADHip_CalculateEncodedSize", "AADHip_EncodePlanCreate",
    "AADHip_EncodePlanDestroy", "AADHip_EncodePlanRun", "AADHip_DecodePlanCreate", "AADHip_DecodePlanDestroy",
    "AADHip_DecodePlanRun", "AADHip_EncodeBatch", "AADHip_DecodeBatch",
    "AADHip_ReconstructPlanCreate", "AADHip_ReconstructPlanDestroy", "AADHip_ReconstructPlanRun",
    "AADHip_ReconstructBatch", "AADHip_SegmentedEncodePlanCreate", "AADHip_SegmentedEncodeBatch",
    "AADHip_SegmentedReconstructPlanCreate", "AADHip_SegmentedReconstructBatch",
    "AADHip_WindowDecodePlanCreate", "AADHip_WindowDecodePlanDestroy", "AADHip_WindowDecodePlanRun",
    "AADHip_WindowDecodePlanRunStats", "AADHip_WindowDecodePlanRunGain", "AADHip_WindowDecodePlanRunPlaced", "AADHip_WindowDecodePlanRunPlacedStats",
    "AADHip_MixedWindowDecodePlanCreate", "AADHip_ChannelMixWindowDecodePlanCreate",
    "AADHip_PlanarEncodePlanCreate", "AADHip_PlanarEncodePlanRun",
    "AADHip_PlanarReconstructPlanCreate", "AADHip_PlanarReconstructPlanRun", "AADHip_PlanarReconstructPlanRunStats",
    "AADHip_WindowReconstructPlanCreate", "AADHip_WindowReconstructPlanDestroy", "AADHip_WindowReconstructPlanRun",
    "AADHip_ResamplerCreate", "AADHip_ResamplerDestroy", "AADHip_ResamplerBank", "AADHip_ResamplerSourceFrames",
    "AADHip_ResamplerResolve", "AADHip_ResamplerRun", "AADHip_ResamplerRunGain", "AADHip_ResamplerRunStats",
    "AADHip_ResamplerCreateWide",
    "AADHip_ConvolverCreate", "AADHip_ConvolverDestroy", "AADHip_ConvolverResponse", "AADHip_ConvolverSourceFrames",
    "AADHip_ConvolverResolve", "AADHip_ConvolverRun", "AADHip_ConvolverRunGain", "AADHip_ConvolverRunStats",
    "AADHip_SpectrogramCreate", "AADHip_SpectrogramDestroy", "AADHip_SpectrogramFrames", "AADHip_SpectrogramCoefficients",
    "AADHip_SpectrogramRun", "AADHip_SpectrogramRunMix",
]
WAV_SYMBOLS = ["AADWav_ParseHeader", "AADWav_WriteHeader", "AADWav_ConvertToPcm16"]
SYNTH_SYMBOLS = ["AADSynth_Generate"]


class AADWavInfo(C.Structure):  # include/aad_wav.h
    _fields_ = [("format_tag", C.c_uint16), ("num_channels", C.c_uint16), ("sampling_rate", C.c_uint32),
                ("bits_per_sample", C.c_uint16), ("num_samples", C.c_uint32), ("data_offset", C.c_uint64),
                ("data_size", C.c_uint64)]


def _declare_legacy(lib):
    u8p, i32pp = C.POINTER(C.c_uint8), C.POINTER(C.POINTER(C.c_int32))
    lib.AADEncoder_CalculateBlockSize.argtypes = [C.c_uint16, C.c_uint16, C.c_uint32,
                                                  C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)]
    lib.AADEncoder_CalculateBlockSize.restype = C.c_int
    lib.AADEncoder_EncodeHeader.argtypes = [C.POINTER(AADHeaderInfo), u8p, C.c_uint32]
    lib.AADEncoder_EncodeHeader.restype = C.c_int
    lib.AADEncoder_CalculateWorkSize.argtypes = [C.c_uint16]
    lib.AADEncoder_CalculateWorkSize.restype = C.c_int32
    lib.AADEncoder_Create.argtypes = [C.c_uint16, C.c_void_p, C.c_int32]
    lib.AADEncoder_Create.restype = C.c_void_p
    lib.AADEncoder_Destroy.argtypes = [C.c_void_p]
    lib.AADEncoder_Destroy.restype = None
    lib.AADEncoder_SetEncodeParameter.argtypes = [C.c_void_p, C.POINTER(AADEncodeParameter)]
    lib.AADEncoder_SetEncodeParameter.restype = C.c_int
    lib.AADEncoder_EncodeWhole.argtypes = [C.c_void_p, i32pp, C.c_uint32, u8p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.AADEncoder_EncodeWhole.restype = C.c_int
    lib.AADDecoder_DecodeHeader.argtypes = [u8p, C.c_uint32, C.POINTER(AADHeaderInfo)]
    lib.AADDecoder_DecodeHeader.restype = C.c_int
    lib.AADDecoder_CalculateWorkSize.argtypes = []
    lib.AADDecoder_CalculateWorkSize.restype = C.c_int32
    lib.AADDecoder_Create.argtypes = [C.c_void_p, C.c_int32]
    lib.AADDecoder_Create.restype = C.c_void_p
    lib.AADDecoder_Destroy.argtypes = [C.c_void_p]
    lib.AADDecoder_Destroy.restype = None
    lib.AADDecoder_SetHeader.argtypes = [C.c_void_p, C.POINTER(AADHeaderInfo)]
    lib.AADDecoder_SetHeader.restype = C.c_int
    lib.AADDecoder_DecodeBlock.argtypes = [C.c_void_p, u8p, C.c_uint32, i32pp, C.c_uint32, C.c_uint32,
                                           C.POINTER(C.c_uint32)]
    lib.AADDecoder_DecodeBlock.restype = C.c_int
    lib.AADDecoder_DecodeWhole.argtypes = [C.c_void_p, u8p, C.c_uint32, i32pp, C.c_uint32, C.c_uint32]
    lib.AADDecoder_DecodeWhole.restype = C.c_int


def _declare_hip(lib):
    vp = C.c_void_p
    lib.AADHip_GetDeviceCount.argtypes = []
    lib.AADHip_GetDeviceCount.restype = C.c_int32
    lib.AADHip_ContextCreate.argtypes = [C.c_int32, vp, C.POINTER(vp)]
    lib.AADHip_ContextCreate.restype = C.c_int
    lib.AADHip_ContextDestroy.argtypes = [vp]
    lib.AADHip_ContextDestroy.restype = None
    lib.AADHip_ContextSynchronize.argtypes = [vp]
    lib.AADHip_ContextSynchronize.restype = C.c_int
    lib.AADHip_ContextLastError.argtypes = [vp]
    lib.AADHip_ContextLastError.restype = C.c_char_p
    lib.AADHip_ContextSignalNextRun.argtypes = [vp, vp, vp]
    lib.AADHip_ContextSignalNextRun.restype = C.c_int
    lib.AADHip_SignalNextRunSupported.argtypes = []
    lib.AADHip_SignalNextRunSupported.restype = C.c_int32
    lib.AADHip_ContextSetOption.argtypes = [vp, C.c_int32, C.c_int32]
    lib.AADHip_ContextSetOption.restype = C.c_int
    lib.AADHip_CalculateEncodedSize.argtypes = [C.POINTER(AADEncodeParameter), C.c_uint32]
    lib.AADHip_CalculateEncodedSize.restype = C.c_uint64
    lib.AADHip_EncodePlanCreate.argtypes = [vp, C.POINTER(AADEncodeParameter), C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_EncodePlanCreate.restype = C.c_int
    lib.AADHip_SegmentedEncodePlanCreate.argtypes = [vp, C.POINTER(AADEncodeParameter), C.POINTER(AADHipSegmentation), C.c_uint32, vp,
                                                     C.POINTER(vp)]
    lib.AADHip_SegmentedEncodePlanCreate.restype = C.c_int
    lib.AADHip_PlanarEncodePlanCreate.argtypes = [vp, C.POINTER(AADEncodeParameter), C.POINTER(AADHipPlanarLayout),
                                                  C.POINTER(AADHipSegmentation), C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_PlanarEncodePlanCreate.restype = C.c_int
    lib.AADHip_PlanarEncodePlanRun.argtypes = [vp, vp, vp, vp]
    lib.AADHip_PlanarEncodePlanRun.restype = C.c_int
    lib.AADHip_PlanarReconstructPlanCreate.argtypes = [vp, C.POINTER(AADEncodeParameter), C.POINTER(AADHipPlanarLayout),
                                                       C.POINTER(AADHipPlanarOutput), C.POINTER(AADHipSegmentation), C.c_uint32, vp,
                                                       C.POINTER(vp)]
    lib.AADHip_PlanarReconstructPlanCreate.restype = C.c_int
    lib.AADHip_PlanarReconstructPlanRun.argtypes = [vp, vp, vp, vp, vp]
    lib.AADHip_PlanarReconstructPlanRun.restype = C.c_int
    lib.AADHip_PlanarReconstructPlanRunStats.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.AADHip_PlanarReconstructPlanRunStats.restype = C.c_int
    lib.AADHip_WindowReconstructPlanCreate.argtypes = [vp, C.POINTER(AADEncodeParameter), C.POINTER(AADHipPlanarLayout),
                                                       C.POINTER(AADHipSegmentation), C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_WindowReconstructPlanCreate.restype = C.c_int
    lib.AADHip_WindowReconstructPlanDestroy.argtypes = [vp]
    lib.AADHip_WindowReconstructPlanDestroy.restype = None
    lib.AADHip_WindowReconstructPlanRun.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, vp, C.POINTER(AADHipPlanarOutput),
                                                    vp, vp]
    lib.AADHip_WindowReconstructPlanRun.restype = C.c_int
    lib.AADHip_EncodePlanDestroy.argtypes = [vp]
    lib.AADHip_EncodePlanDestroy.restype = None
    lib.AADHip_EncodePlanRun.argtypes = [vp, vp, vp, vp]
    lib.AADHip_EncodePlanRun.restype = C.c_int
    lib.AADHip_DecodePlanCreate.argtypes = [vp, C.POINTER(AADHeaderInfo), C.c_int32, C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_DecodePlanCreate.restype = C.c_int
    lib.AADHip_DecodePlanDestroy.argtypes = [vp]
    lib.AADHip_DecodePlanDestroy.restype = None
    lib.AADHip_DecodePlanRun.argtypes = [vp, vp, vp]
    lib.AADHip_DecodePlanRun.restype = C.c_int
    lib.AADHip_WindowDecodePlanCreate.argtypes = [vp, C.POINTER(AADHeaderInfo), C.c_int32, C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_WindowDecodePlanCreate.restype = C.c_int
    lib.AADHip_MixedWindowDecodePlanCreate.argtypes = [vp, C.c_uint32, C.c_int32, C.c_uint32, vp, vp, C.POINTER(vp)]
    lib.AADHip_MixedWindowDecodePlanCreate.restype = C.c_int
    lib.AADHip_ChannelMixWindowDecodePlanCreate.argtypes = [vp, C.c_uint32, C.c_int32, C.c_uint32, vp, vp, C.POINTER(vp)]
    lib.AADHip_ChannelMixWindowDecodePlanCreate.restype = C.c_int
    lib.AADHip_WindowDecodePlanDestroy.argtypes = [vp]
    lib.AADHip_WindowDecodePlanDestroy.restype = None
    lib.AADHip_WindowDecodePlanRun.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp]
    lib.AADHip_WindowDecodePlanRun.restype = C.c_int
    lib.AADHip_WindowDecodePlanRunStats.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp, vp]
    lib.AADHip_WindowDecodePlanRunStats.restype = C.c_int
    lib.AADHip_WindowDecodePlanRunGain.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int32, vp, vp, C.c_int32]
    lib.AADHip_WindowDecodePlanRunGain.restype = C.c_int
    lib.AADHip_WindowDecodePlanRunPlaced.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_int32, vp, vp, C.c_int32]
    lib.AADHip_WindowDecodePlanRunPlaced.restype = C.c_int
    lib.AADHip_WindowDecodePlanRunPlacedStats.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint32, vp]
    lib.AADHip_WindowDecodePlanRunPlacedStats.restype = C.c_int
    lib.AADHip_ResamplerCreate.argtypes = [vp, C.c_uint32, C.POINTER(AADHipResampleRatio), C.c_uint32, C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_ResamplerCreate.restype = C.c_int
    lib.AADHip_ResamplerCreateWide.argtypes = list(lib.AADHip_ResamplerCreate.argtypes)
    lib.AADHip_ResamplerCreateWide.restype = C.c_int
    lib.AADHip_ResamplerDestroy.argtypes = [vp]
    lib.AADHip_ResamplerDestroy.restype = None
    lib.AADHip_ResamplerBank.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, C.c_uint64]
    lib.AADHip_ResamplerBank.restype = C.c_int
    lib.AADHip_ResamplerSourceFrames.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.AADHip_ResamplerSourceFrames.restype = C.c_int
    lib.AADHip_ResamplerResolve.argtypes = [vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp]
    lib.AADHip_ResamplerResolve.restype = C.c_int
    lib.AADHip_ResamplerRun.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_int32, vp]
    lib.AADHip_ResamplerRun.restype = C.c_int
    lib.AADHip_ResamplerRunGain.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_int32, vp, vp, C.c_int32]
    lib.AADHip_ResamplerRunGain.restype = C.c_int
    lib.AADHip_ResamplerRunStats.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_int32, vp, vp]
    lib.AADHip_ResamplerRunStats.restype = C.c_int
    lib.AADHip_ConvolverCreate.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(vp)]
    lib.AADHip_ConvolverCreate.restype = C.c_int
    lib.AADHip_ConvolverDestroy.argtypes = [vp]
    lib.AADHip_ConvolverDestroy.restype = None
    lib.AADHip_ConvolverResponse.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, C.c_uint64]
    lib.AADHip_ConvolverResponse.restype = C.c_int
    lib.AADHip_ConvolverSourceFrames.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.AADHip_ConvolverSourceFrames.restype = C.c_int
    lib.AADHip_ConvolverResolve.argtypes = [vp, C.c_uint64, vp, vp, C.c_uint32, vp, vp]
    lib.AADHip_ConvolverResolve.restype = C.c_int
    lib.AADHip_ConvolverRun.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_int32, vp]
    lib.AADHip_ConvolverRun.restype = C.c_int
    lib.AADHip_ConvolverRunGain.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_int32, vp, vp, C.c_int32]
    lib.AADHip_ConvolverRunGain.restype = C.c_int
    lib.AADHip_ConvolverRunStats.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_int32, vp, vp]
    lib.AADHip_ConvolverRunStats.restype = C.c_int
    lib.AADHip_SpectrogramCreate.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_SpectrogramCreate.restype = C.c_int
    lib.AADHip_SpectrogramDestroy.argtypes = [vp]
    lib.AADHip_SpectrogramDestroy.restype = None
    lib.AADHip_SpectrogramFrames.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.AADHip_SpectrogramFrames.restype = C.c_int
    lib.AADHip_SpectrogramCoefficients.argtypes = [vp, C.POINTER(C.c_uint32), vp, C.c_uint64]
    lib.AADHip_SpectrogramCoefficients.restype = C.c_int
    lib.AADHip_SpectrogramRun.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp]
    lib.AADHip_SpectrogramRun.restype = C.c_int
    lib.AADHip_SpectrogramRunMix.argtypes = [vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint32, vp]
    lib.AADHip_SpectrogramRunMix.restype = C.c_int
    lib.AADHip_EncodeBatch.argtypes = [vp, C.POINTER(AADEncodeParameter), C.c_uint32, vp, vp, vp, vp, vp, vp]
    lib.AADHip_EncodeBatch.restype = C.c_int
    lib.AADHip_DecodeBatch.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp]
    lib.AADHip_DecodeBatch.restype = C.c_int
    lib.AADHip_ReconstructPlanCreate.argtypes = [vp, C.POINTER(AADEncodeParameter), C.c_uint32, vp, C.POINTER(vp)]
    lib.AADHip_ReconstructPlanCreate.restype = C.c_int
    lib.AADHip_ReconstructPlanDestroy.argtypes = [vp]
    lib.AADHip_ReconstructPlanDestroy.restype = None
    lib.AADHip_ReconstructPlanRun.argtypes = [vp, vp, vp, vp, C.c_int32, vp]
    lib.AADHip_ReconstructPlanRun.restype = C.c_int
    lib.AADHip_ReconstructBatch.argtypes = [vp, C.POINTER(AADEncodeParameter), C.c_uint32, vp, vp, C.c_int32, vp, vp]
    lib.AADHip_ReconstructBatch.restype = C.c_int
    lib.AADHip_SegmentedEncodeBatch.argtypes = [vp, C.POINTER(AADEncodeParameter), C.POINTER(AADHipSegmentation), C.c_uint32, vp, vp,
                                                vp, vp, vp]
    lib.AADHip_SegmentedEncodeBatch.restype = C.c_int
    lib.AADHip_SegmentedReconstructPlanCreate.argtypes = [vp, C.POINTER(AADEncodeParameter), C.POINTER(AADHipSegmentation), C.c_uint32,
                                                          vp, C.POINTER(vp)]
    lib.AADHip_SegmentedReconstructPlanCreate.restype = C.c_int
    lib.AADHip_SegmentedReconstructBatch.argtypes = [vp, C.POINTER(AADEncodeParameter), C.POINTER(AADHipSegmentation), C.c_uint32, vp,
                                                     vp, C.c_int32, vp, vp]
    lib.AADHip_SegmentedReconstructBatch.restype = C.c_int
    lib.AADWav_ParseHeader.argtypes = [vp, C.c_uint64, C.POINTER(AADWavInfo)]
    lib.AADWav_ParseHeader.restype = C.c_int
    lib.AADWav_WriteHeader.argtypes = [vp, C.c_uint32, C.c_uint16, C.c_uint32, C.c_uint32]
    lib.AADWav_WriteHeader.restype = C.c_int
    lib.AADWav_ConvertToPcm16.argtypes = [vp, C.c_uint16, C.c_uint64, vp]
    lib.AADWav_ConvertToPcm16.restype = C.c_int


def load_library(path=None, hip=True):
    """Load a library exporting the AAD C API.  The product library must exist: there is no
    fallback of any kind (build it with ``python -c 'import __graft_entry__ as g; g.build()'``)."""
    path = path or LIBRARY_PATH
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s is missing - the HIP extension has not been built (run __graft_entry__.build())" % path)
    if hip:
        # torch ships a HIP runtime of its own.  Whichever libamdhip64 is mapped first serves both; loaded
        # the other way round (this library first, torch later) the process ends up with two runtimes and
        # AADHip_ContextCreate fails - so python callers that have torch get it imported here.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(path)
    _declare_legacy(lib)
    if hip:
        _declare_hip(lib)
    return lib


def make_parameter(channels, bits, max_block_size=1024, rate=48000, ms=False, trials=0):
    return AADEncodeParameter(num_channels=channels, sampling_rate=rate, bits_per_sample=bits,
                              max_block_size=max_block_size, ch_process_method=1 if ms else 0,
                              num_encode_trials=trials)


def _planar_pointers(planar):
    """planar: int32 array [channels, samples] (C-contiguous) -> int32** for the legacy API"""
    rows = (C.POINTER(C.c_int32) * planar.shape[0])()
    for c in range(planar.shape[0]):
        rows[c] = planar[c].ctypes.data_as(C.POINTER(C.c_int32))
    return rows


class ApiError(RuntimeError):
    def __init__(self, where, code):
        super().__init__("%s -> %s" % (where, AADApiResult.name(code)))
        self.code = int(code)


class LegacyCodec:
    """The reference's call sequences (src/main.c:91-106, 182-198) against a loaded library."""

    def __init__(self, lib):
        self.lib = lib

    def block_size(self, max_block_size, channels, bits):
        bs, spb = C.c_uint16(0), C.c_uint32(0)
        rc = self.lib.AADEncoder_CalculateBlockSize(max_block_size, channels, bits, C.byref(bs), C.byref(spb))
        return rc, bs.value, spb.value

    def encode(self, pcm, bits=4, max_block_size=1024, rate=48000, ms=False, trials=0, encoder=None,
               capacity=None):
        """pcm: int16/int32 array [samples, channels] -> bytes of the .aad image."""
        pcm = np.asarray(pcm)
        n, ch = pcm.shape
        planar = np.ascontiguousarray(pcm.T.astype(np.int32))
        param = make_parameter(ch, bits, max_block_size, rate, ms, trials)
        own = encoder is None
        if own:
            encoder = self.lib.AADEncoder_Create(max_block_size, None, 0)
            if not encoder:
                raise ApiError("AADEncoder_Create", AADApiResult.NG)
        try:
            rc = self.lib.AADEncoder_SetEncodeParameter(encoder, C.byref(param))
            if rc != 0:
                raise ApiError("AADEncoder_SetEncodeParameter", rc)
            cap = int(capacity) if capacity is not None else max(64, n * ch * 2 + 64 + 18 * ch * (n // 4 + 2))
            out = np.zeros(cap, dtype=np.uint8)
            size = C.c_uint32(0)
            rc = self.lib.AADEncoder_EncodeWhole(encoder, _planar_pointers(planar), n,
                                                 out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(size))
            if rc != 0:
                raise ApiError("AADEncoder_EncodeWhole", rc)
            return out[:size.value].tobytes()
        finally:
            if own:
                self.lib.AADEncoder_Destroy(encoder)

    def decode_header(self, data):
        buf = np.frombuffer(data, dtype=np.uint8)
        h = AADHeaderInfo()
        rc = self.lib.AADDecoder_DecodeHeader(buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), C.byref(h))
        if rc != 0:
            raise ApiError("AADDecoder_DecodeHeader", rc)
        return h

    def decode(self, data):
        """bytes of an .aad image -> (int16 array [samples, channels], header)"""
        h = self.decode_header(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        planar = np.zeros((h.num_channels, h.num_samples), dtype=np.int32)
        dec = self.lib.AADDecoder_Create(None, 0)
        try:
            rc = self.lib.AADDecoder_DecodeWhole(dec, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf),
                                                 _planar_pointers(planar), h.num_channels, h.num_samples)
            if rc != 0:
                raise ApiError("AADDecoder_DecodeWhole", rc)
        finally:
            self.lib.AADDecoder_Destroy(dec)
        return np.ascontiguousarray(planar.T).astype(np.int16), h

    def decode_block(self, header, block, want_samples):
        buf = np.frombuffer(block, dtype=np.uint8)
        planar = np.zeros((header.num_channels, max(want_samples, 1)), dtype=np.int32)
        got = C.c_uint32(0)
        dec = self.lib.AADDecoder_Create(None, 0)
        try:
            rc = self.lib.AADDecoder_SetHeader(dec, C.byref(header))
            if rc != 0:
                raise ApiError("AADDecoder_SetHeader", rc)
            rc = self.lib.AADDecoder_DecodeBlock(dec, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf),
                                                 _planar_pointers(planar), header.num_channels, want_samples,
                                                 C.byref(got))
            if rc != 0:
                raise ApiError("AADDecoder_DecodeBlock", rc)
        finally:
            self.lib.AADDecoder_Destroy(dec)
        return np.ascontiguousarray(planar[:, :got.value].T).astype(np.int16)
