"""The case table of every kernel but the window decoders: each instantiation that an entry point of include/aad_hip.h can reach,
written down from the dispatch code.  Nothing here is read from the built library: tests/test_encode_kernel_census.py compares
this table with the kernels the library holds, and tests/test_gpu_encode_matrix.py runs the case each encoder and decoder record
names (the window decoders: tests/window_matrix.py).

The encoders - encode_streams_kernel<BITS, CHF, MS, QUAD, TRIALS, DUAL, RING, SEG, IN, REC> (aad_amd/csrc/aad_encode.hip.h):
  run_encode (aad_hip_engine.hip)         REC by EncodeRun::rec, IN by EncodeRun::in: launch_encode_run<IN, REC>.  The pairs that
                                          exist: <interleaved, none> in aad_hip_engine.hip, every other one by the extern template
                                          list of aad_encode_launch.hip.h = the objects of aad_encode_units.hip
  launch_encode_run                       SEG by EncodeRun::chain_table, BITS by args.bits: 4, 3, anything else
  launch_encode                           (QUAD, TRIALS, DUAL, RING) by the plan: trials ? (quad-dual | quad | dense) :
                                          (quad | dense-ring | dense); quad-dual and dense-ring without a REC, dense-ring without SEG
  launch_encode_mapped                    (CHF, MS) by channels and mid_side: mono (not for planar int16 rows: they are interleaved
                                          frames), then - not for <interleaved, REC>, which serves mono int16 rows alone - M/S, L/R and,
                                          on the dense ring-free kernels, any channel count (CHF = 0)
The decoders:
  decode_blocks_kernel<BITS, CHF, MS, QUAD, NT>      launch_decode_mapped (aad_hip_engine.hip): QUAD mono / M/S / L/R; dense those
                                                     and CHF = 0; NT (streamed stores) dense stereo at 4 and 2 bits alone
  decode_split_kernel<BITS, CHF, MS, LDSRES, ROLE>   launch_decode_split -> launch_bits (aad_decode_split.hip)
  decode_tiled_kernel<BITS, CHF, MS>                 launch_decode_tiled -> launch_bits (aad_decode_tiled.hip)
The rest - compare_*, window_resolve_kernel, the resamplers - get records that point at the existing GPU test that runs them.

A record is (kernel, args, case): the kernel's name in namespace aad, its template arguments in the order of the C++ parameter
list with defaults written out (bool as 0 / 1, enums by value), and where it runs: an id of tests/test_gpu_encode_matrix.py, or
"<file>::<test function>" of an existing GPU test.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
from collections import namedtuple

Cell = namedtuple("Cell", "kernel args case")

GPU_FILE = "test_gpu_encode_matrix.py"

BITS = (4, 3, 2)                                     # the bits switches' rungs: 4, 3, anything else
IN_INTERLEAVED, IN_PLANAR_I16, IN_PLANAR_F32 = 0, 1, 2  # enum PcmLayout
REC_NONE, REC_I16, REC_F32, REC_I16_STATS, REC_F32_STATS, REC_STATS_ONLY = range(6)  # enum RecOutput
SAMPLE_INT16, SAMPLE_FLOAT32, SAMPLE_FLOAT16, SAMPLE_BFLOAT16 = 0, 1, 4, 5  # enum AADHipSampleType
RESAMPLE_NO_ROWS = -1                                # kResampleNoRows: ST of the statistics-only resamplers

IN_NAMES = {IN_INTERLEAVED: "frames", IN_PLANAR_I16: "i16rows", IN_PLANAR_F32: "f32rows"}
REC_NAMES = {REC_NONE: "images", REC_I16: "i16", REC_F32: "f32", REC_I16_STATS: "i16stats", REC_F32_STATS: "f32stats",
             REC_STATS_ONLY: "stats"}

# launch_encode_run<IN, REC>'s instantiations: aad_hip_engine.hip holds <interleaved, none>; aad_encode_units.hip, compiled per
# (AAD_ENCODE_IN_F32, AAD_ENCODE_REC), the planar pair and - int16 input with a REC - the interleaved one beside it
ENCODE_PAIRS = [(IN_INTERLEAVED, REC_NONE)] + \
               [(i, r) for r in range(6) for i in ((IN_INTERLEAVED,) if r else ()) + (IN_PLANAR_I16, IN_PLANAR_F32)]


def encode_variants(seg, rec):
    """launch_encode's branches as (QUAD, TRIALS, DUAL, RING), in its order"""
    out = []
    if rec == REC_NONE:
        out.append((1, 1, 1, 0))          # p.trials, EncodeKernel::QuadDual; with a REC: never planned, no instantiation
    out += [(1, 1, 0, 0), (0, 1, 0, 0)]   # p.trials: Quad, else
    out.append((1, 0, 0, 0))              # Quad
    if not seg and rec == REC_NONE:
        out.append((0, 0, 0, 1))          # DenseRing; SEG: ring_ok = 0, REC: never planned
    out.append((0, 0, 0, 0))              # else
    return out


def encode_rungs(variant, inp, rec):
    """launch_encode_mapped's rungs as (CHF, MS, QUAD, DUAL, RING): the any-channel kernel drops QUAD, DUAL and RING"""
    quad, _, dual, ring = variant
    out = []
    if inp != IN_PLANAR_I16:
        out.append((1, 0, quad, dual, ring))
    if inp == IN_INTERLEAVED and rec != REC_NONE:
        return out
    out += [(2, 1, quad, dual, ring), (2, 0, quad, dual, ring)]
    if not quad and not ring:
        out.append((0, 0, 0, 0, 0))
    return out


def encode_group_id(group):
    inp, rec, seg, bits = group
    return "%s-%s-%s-%db" % (IN_NAMES[inp], REC_NAMES[rec], "chains" if seg else "serial", bits)


def encode_case(inp, rec, seg, bits):
    return "test_encoder_kernels[%s]" % encode_group_id((inp, rec, seg, bits))


def encode_groups():
    """[(IN, REC, SEG, BITS)]: the parametrised cases of the encoder"""
    return [(i, r, s, b) for i, r in ENCODE_PAIRS for s in (0, 1) for b in BITS]


def encode_cells_of(group):
    inp, rec, seg, bits = group
    out = []
    for v in encode_variants(seg, rec):
        for chf, ms, quad, dual, ring in encode_rungs(v, inp, rec):
            out.append(Cell("encode_streams_kernel", (bits, chf, ms, quad, v[1], dual, ring, seg, inp, rec), encode_case(inp, rec, seg, bits)))
    return out


# ---- the decoders --------------------------------------------------------------------------------------------------------------------
DECODE_FAMILIES = ("blocks", "split", "tiled")
THREE_RUNGS = ((1, 0), (2, 1), (2, 0))                # channels == 1; mid_side; anything else (stereo)


def decode_group_id(group):
    return "%s-%db" % group


def decode_case(family, bits):
    return "test_decoder_kernels[%s]" % decode_group_id((family, bits))


def decode_groups():
    return [(f, b) for f in DECODE_FAMILIES for b in BITS]


def decode_cells_of(group):
    family, bits = group
    case = decode_case(family, bits)
    if family == "blocks":  # launch_decode<BITS>: QuadFused -> launch_decode_mapped<BITS, true>, Dense -> <BITS, false>
        out = [Cell("decode_blocks_kernel", (bits, chf, ms, 1, 0), case) for chf, ms in THREE_RUNGS]
        out += [Cell("decode_blocks_kernel", (bits, chf, ms, 0, 0), case) for chf, ms in THREE_RUNGS + ((0, 0),)]
        if bits != 3:       # p.stream_stores on the dense stereo kernels
            out += [Cell("decode_blocks_kernel", (bits, 2, ms, 0, 1), case) for ms in (1, 0)]
        return out
    if family == "split":   # launch_decode_split: LDSRES by SplitLds / SplitScratch, ROLE by p.simd_role
        return [Cell("decode_split_kernel", (bits, chf, ms, lds, role), case) for lds in (1, 0) for role in (1, 0) for chf, ms in THREE_RUNGS]
    return [Cell("decode_tiled_kernel", (bits, chf, ms), case) for chf, ms in THREE_RUNGS]


# ---- the rest: records that point at the existing GPU test that runs the kernel ----------------------------------------------------
ROW_TYPES = (SAMPLE_INT16, SAMPLE_FLOAT32, SAMPLE_FLOAT16, SAMPLE_BFLOAT16)   # launch_resample_rows: three cases and default
GAIN_TYPES = (SAMPLE_FLOAT32, SAMPLE_FLOAT16, SAMPLE_BFLOAT16)                # launch_resample_rows_gain: two cases and default
STATS_TYPES = (RESAMPLE_NO_ROWS,) + ROW_TYPES                                 # launch_resample_rows_stats: out == nullptr first


def other_cells():
    plain, mix, wide = "test_gpu_window_resample.py", "test_gpu_resample_mix.py", "test_gpu_resample_wide.py"
    out = [
        Cell("compare_segments_kernel", (), "test_gpu_reconstruct.py::test_reconstruct_device_resident_vs_oracle"),
        Cell("compare_finish_kernel", (), "test_gpu_reconstruct.py::test_reconstruct_device_resident_vs_oracle"),
        Cell("window_resolve_kernel", (), "test_gpu_window_reconstruct.py::test_channels_bits_and_segmentations"),
        Cell("resample_resolve_kernel", (), plain + "::test_rows_equal_the_definition"),
    ]
    out += [Cell("resample_rows_kernel", (st,), plain + "::test_rows_equal_the_definition") for st in ROW_TYPES]
    out += [Cell("resample_rows_gain_kernel", (st, add), mix + "::test_rows_with_gain_store_and_add") for st in GAIN_TYPES for add in (1, 0)]
    out += [Cell("resample_rows_stats_kernel", (st,), mix + "::test_statistics") for st in STATS_TYPES]
    out += [Cell("resample_rows_wide_kernel", (st,), wide + "::test_rows_equal_the_definition") for st in ROW_TYPES]
    out += [Cell("resample_rows_gain_wide_kernel", (st, add), wide + "::test_rows_with_gain_store_and_add") for st in GAIN_TYPES for add in (1, 0)]
    out += [Cell("resample_rows_stats_wide_kernel", (st,), wide + "::test_statistics") for st in STATS_TYPES]
    return out


# kernels the library holds that no entry point reaches, (kernel, args) -> the reason, which names the host line that rules it out.
# The census fails on any other surplus.  Empty: launch_encode and launch_encode_mapped leave out with `if constexpr` exactly what
# the plans (aad_launch_policy.h) and run_encode never name, and every rung that is left is named by a plan some entry point accepts.
UNREACHABLE = {}

# reachable instantiations per kernel, pinned as literal numbers (test_encode_kernel_census.py holds them to the table and the library)
COUNTS = {
    "encode_streams_kernel": 1140,
    "decode_blocks_kernel": 25,
    "decode_split_kernel": 36,
    "decode_tiled_kernel": 9,
    "compare_segments_kernel": 1,
    "compare_finish_kernel": 1,
    "window_resolve_kernel": 1,
    "resample_resolve_kernel": 1,
    "resample_rows_kernel": 4,
    "resample_rows_gain_kernel": 6,
    "resample_rows_stats_kernel": 5,
    "resample_rows_wide_kernel": 4,
    "resample_rows_gain_wide_kernel": 6,
    "resample_rows_stats_wide_kernel": 5,
}


def matrix_cells():
    """the records test_gpu_encode_matrix.py launches: encoders and decoders"""
    out = []
    for g in encode_groups():
        out += encode_cells_of(g)
    for g in decode_groups():
        out += decode_cells_of(g)
    return out


def cells():
    """one record per reachable kernel instantiation that is no window decoder"""
    out = matrix_cells() + other_cells()
    assert len({(c.kernel, c.args) for c in out}) == len(out)
    return out
