"""The case table of window decode: every kernel instantiation that the entry points of include/aad_hip.h can reach
(AADHip_WindowDecodePlanRun, ...RunStats, ...RunGain, ...RunPlaced, ...RunPlacedStats over same-format, mixed-format and
channel-mix plans), written down from the dispatch code of the fifteen translation units aad_amd/csrc/aad_decode_window*.hip -
the launch nest and the objects' sample types of aad_amd/csrc/aad_window_unit.hip.h - and the half / not-half switch of
launch_window_unit (aad_amd/csrc/aad_launch.h).  Nothing here is read from the built library: tests/test_window_kernel_census.py compares this table
with the kernels the library holds, and tests/test_gpu_window_decode_matrix.py runs the case each record names.

A record is (kernel, args, case): the kernel's name in namespace aad, its template arguments in the order of the C++ parameter
list - BITS, CHF (1 / 2: the mono / stereo fast paths, 0: any channel count), MS, then the sample type number where the kernel has
one, then OUTC for a channel mix - and the id of the test case of the GPU file that launches it.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
from collections import namedtuple

from aad_amd.capi import SAMPLE_BFLOAT16, SAMPLE_FLOAT16, SAMPLE_FLOAT32, SAMPLE_INT16

Cell = namedtuple("Cell", "kernel args case")

GPU_FILE = "test_gpu_window_decode_matrix.py"

BITS = (4, 3, 2)                                      # launch_window_bits' rungs: 4, 3, anything else
# launch_window_channels' rungs as (CHF, MS): channels == 1; channels == 2 && mid_side; channels == 2; anything else
FOUR_RUNGS = ((1, 0), (2, 1), (2, 0), (0, 0))
# a channel mix knows one and two channels: channels == 1; mid_side; anything else
THREE_RUNGS = ((1, 0), (2, 1), (2, 0))
OUT_CHANNELS = (1, 2)                                 # launch_window_out: out_channels == 1, anything else

# the sample types of a unit's two objects: WindowUnitTypes<MODE, false> and <MODE, true>; the gain and placed units hold
# float32 alone in their first object (AAD_WINDOW_HALF=0) and float16 / bfloat16 in their second
ROW_TYPES = (SAMPLE_INT16, SAMPLE_FLOAT32, SAMPLE_FLOAT16, SAMPLE_BFLOAT16)
GAIN_TYPES = (SAMPLE_FLOAT32, SAMPLE_FLOAT16, SAMPLE_BFLOAT16)
NO_TYPE = (None,)                                     # the _placed_stats units write no rows: one object, no ST parameter

# ---- the matrix cases of the GPU file ----------------------------------------------------------------------------------------------
# same-format plans: (channels, bits, mid/side)
GEOMETRIES = [(c, b, ms) for c, ms in ((1, False), (2, False), (2, True), (3, False)) for b in BITS]
# mixed plans by channel count: the (bits, mid/side) variants among their streams
MIXED_PLANS = {
    "mono": (1, [(b, False) for b in BITS]),
    "stereo": (2, [(b, ms) for b in BITS for ms in (False, True)]),
    "3ch": (3, [(b, False) for b in BITS]),
}
# the channel-mix corpus: (source channels, bits, mid/side), all nine
CHANNEL_VARIANTS = [(1, b, False) for b in BITS] + [(2, b, ms) for b in BITS for ms in (False, True)]


def geometry_id(g):
    return "%dch%db%s" % (g[0], g[1], "ms" if g[2] else "")


def out_channels_id(oc):
    return "to_mono" if oc == 1 else "to_stereo"


def same_format_case(bits, chf, ms):
    return "test_same_format_plans[%s]" % geometry_id((chf if chf else 3, bits, bool(ms)))


def mixed_case(chf):
    return "test_mixed_plans[%s]" % {1: "mono", 2: "stereo", 0: "3ch"}[chf]


def channel_mix_case(outc):
    return "test_channel_mix_plans[%s]" % out_channels_id(outc)


# ---- one helper per unit kind ------------------------------------------------------------------------------------------------------
def _args(bits, chf, ms, st, outc=None):
    return (bits, chf, ms) + (() if st is None else (st,)) + (() if outc is None else (outc,))


def _same_format_unit(kernel, types):
    """aad_decode_window.hip, _stats, _gain, _placed, _placed_stats: launch_type -> launch_bits"""
    return [Cell(kernel, _args(b, chf, ms, st), same_format_case(b, chf, ms)) for st in types for b in BITS for chf, ms in FOUR_RUNGS]


def _mixed_unit(kernel, types):
    """aad_decode_window_mixed.hip and its four siblings: the same ladders, one launch per variant of the plan"""
    return [Cell(kernel, _args(b, chf, ms, st), mixed_case(chf)) for st in types for b in BITS for chf, ms in FOUR_RUNGS]


def _channel_mix_unit(kernel, types):
    """aad_decode_window_channel_mix.hip and its four siblings: launch_rows / the unit function pick OUTC, then the ladders"""
    return [Cell(kernel, _args(b, chf, ms, st, oc), channel_mix_case(oc))
            for oc in OUT_CHANNELS for st in types for b in BITS for chf, ms in THREE_RUNGS]


# (translation unit, kernel, helper, sample types): the fifteen units
UNITS = [
    ("aad_decode_window.hip", "decode_window_kernel", _same_format_unit, ROW_TYPES),
    ("aad_decode_window_mixed.hip", "decode_window_mixed_kernel", _mixed_unit, ROW_TYPES),
    ("aad_decode_window_channel_mix.hip", "decode_window_channel_mix_kernel", _channel_mix_unit, ROW_TYPES),
    ("aad_decode_window_stats.hip", "decode_window_stats_kernel", _same_format_unit, ROW_TYPES),
    ("aad_decode_window_mixed_stats.hip", "decode_window_mixed_stats_kernel", _mixed_unit, ROW_TYPES),
    ("aad_decode_window_channel_mix_stats.hip", "decode_window_channel_mix_stats_kernel", _channel_mix_unit, ROW_TYPES),
    ("aad_decode_window_gain.hip", "decode_window_gain_kernel", _same_format_unit, GAIN_TYPES),
    ("aad_decode_window_mixed_gain.hip", "decode_window_mixed_gain_kernel", _mixed_unit, GAIN_TYPES),
    ("aad_decode_window_channel_mix_gain.hip", "decode_window_channel_mix_gain_kernel", _channel_mix_unit, GAIN_TYPES),
    ("aad_decode_window_placed.hip", "decode_window_placed_kernel", _same_format_unit, GAIN_TYPES),
    ("aad_decode_window_mixed_placed.hip", "decode_window_mixed_placed_kernel", _mixed_unit, GAIN_TYPES),
    ("aad_decode_window_channel_mix_placed.hip", "decode_window_channel_mix_placed_kernel", _channel_mix_unit, GAIN_TYPES),
    ("aad_decode_window_placed_stats.hip", "decode_window_placed_stats_kernel", _same_format_unit, NO_TYPE),
    ("aad_decode_window_mixed_placed_stats.hip", "decode_window_mixed_placed_stats_kernel", _mixed_unit, NO_TYPE),
    ("aad_decode_window_channel_mix_placed_stats.hip", "decode_window_channel_mix_placed_stats_kernel", _channel_mix_unit, NO_TYPE),
]

# kernels the library holds that no entry point reaches, (kernel, args) -> the reason.  The census fails on any other surplus.
# Empty: every rung of every ladder is named by a plan some entry point accepts.
UNREACHABLE = {}


def cells():
    """one record per reachable kernel instantiation"""
    out = []
    for _, kernel, helper, types in UNITS:
        out += helper(kernel, types)
    assert len({(c.kernel, c.args) for c in out}) == len(out)
    return out


def cells_per_unit():
    """translation unit -> number of records"""
    return {unit: len(helper(kernel, types)) for unit, kernel, helper, types in UNITS}
