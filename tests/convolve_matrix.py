"""The convolve stage's kernels (aad_amd/csrc/aad_convolve.hip, namespace aad::convolve), one record per instantiation: the kernel,
its template arguments as they stand in the mangled name, and the case of tests/test_gpu_convolve.py that runs it.
tests/test_convolve_kernel_census.py holds the built library to exactly these records.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import re
from collections import namedtuple

from kernel_names import ARG

GPU_FILE = "test_gpu_convolve.py"
INT16, FLOAT32, FLOAT16, BFLOAT16 = 0, 1, 4, 5  # enum AADHipSampleType
STORE, ADD = 0, 1

Cell = namedtuple("Cell", "kernel args case")

# _ZN3aad8convolve <length> <name> [I <arguments> E] E <parameter types>: kernel_names.NAME with the nested namespace in front; that
# pattern reads "8convolve..." as a name with a wrong length prefix and so never counts these kernels
NAME = re.compile(rb"_ZN3aad8convolve(\d+)([a-z][a-z0-9_]*_kernel)(?:I((?:L[ib]n?\d+E)+)E)?E")


def kernels_in(data):
    """bytes -> the set of (kernel, template arguments) among the mangled names of aad::convolve kernels in them"""
    found = set()
    for m in NAME.finditer(data):
        name = m.group(2)
        if int(m.group(1)) != len(name):
            continue
        found.add((name.decode(), tuple(-int(v) if neg else int(v) for _, neg, v in ARG.findall(m.group(3) or b""))))
    return found


def cells():
    out = [Cell("convolve_resolve_kernel", (), "test_rows_equal_the_definition")]
    out += [Cell("convolve_rows_kernel", (st,), "test_rows_equal_the_definition") for st in (INT16, FLOAT32, FLOAT16, BFLOAT16)]
    out += [Cell("convolve_rows_gain_kernel", (st, add), "test_rows_with_gain_store_and_add")
            for st in (FLOAT32, FLOAT16, BFLOAT16) for add in (STORE, ADD)]
    return out
