"""The convolve stage's statistics kernels (aad_amd/csrc/aad_convolve_stats.hip, namespace aad::convolve_levels), one record per
instantiation: the kernel, its template argument as it stands in the mangled name, and the case of
tests/test_gpu_convolve_stats.py that runs it.  tests/test_convolve_stats_kernel_census.py holds the built library to exactly these
records.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import re
from collections import namedtuple

from kernel_names import ARG

GPU_FILE = "test_gpu_convolve_stats.py"
NO_ROWS, INT16, FLOAT32, FLOAT16, BFLOAT16 = -1, 0, 1, 4, 5  # kNoRows, enum AADHipSampleType

Cell = namedtuple("Cell", "kernel args case")

# _ZN3aad15convolve_levels <length> <name> I <argument> E E <parameter types>: neither kernel_names.NAME nor convolve_matrix.NAME
# reads "15convolve_levels..." as a kernel of theirs
NAME = re.compile(rb"_ZN3aad15convolve_levels(\d+)([a-z][a-z0-9_]*_kernel)(?:I((?:L[ib]n?\d+E)+)E)?E")


def kernels_in(data):
    """bytes -> the set of (kernel, template arguments) among the mangled names of aad::convolve_levels kernels in them"""
    found = set()
    for m in NAME.finditer(data):
        name = m.group(2)
        if int(m.group(1)) != len(name):
            continue
        found.add((name.decode(), tuple(-int(v) if neg else int(v) for _, neg, v in ARG.findall(m.group(3) or b""))))
    return found


def cells():
    return [Cell("convolve_rows_stats_kernel", (st,), "test_statistics_equal_the_definition")
            for st in (NO_ROWS, INT16, FLOAT32, FLOAT16, BFLOAT16)]
