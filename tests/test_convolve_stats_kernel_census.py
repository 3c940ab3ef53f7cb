"""The census of the convolve stage's statistics kernels: the instantiations of namespace aad::convolve_levels that the built
library holds against the records of tests/convolve_stats_matrix.py, the names read from the library's bytes as
tests/kernel_names.py reads them - names only, no code.  The two sets must be EQUAL, five kernels, and every record names a case
of tests/test_gpu_convolve_stats.py.  The older census tests read other namespaces and neither count nor miss these.  No GPU."""
import pytest

import aad_amd
import convolve_matrix as cm
import convolve_stats_matrix as sm
import kernel_names
from aad_amd import capi


@pytest.fixture(scope="module")
def lib():
    return aad_amd.load_library()


def test_the_parser_on_names_written_by_hand():
    data = (b"\0_ZN3aad15convolve_levels26convolve_rows_stats_kernelILin1EEEvNS_8convolve9StatsArgsE\0"
            b"_ZN3aad15convolve_levels41__device_stub__convolve_rows_stats_kernelILi4EEEvNS_8convolve9StatsArgsE\0"
            b"_ZN3aad15convolve_levels26convolve_rows_stats_kernelILi5EEEvNS_8convolve9StatsArgsE\0"
            b"_ZN3aad15convolve_levels25convolve_rows_stats_kernelILi1EEEvNS_8convolve9StatsArgsE\0"  # a wrong length: no name of ours
            b"_ZN3aad8convolve20convolve_rows_kernelILi1EEEvNS0_8RowsArgsE\0")                         # another namespace
    assert sm.kernels_in(data) == {("convolve_rows_stats_kernel", (-1,)), ("convolve_rows_stats_kernel", (5,))}
    # and the patterns of the older census tests see none of the family
    assert kernel_names.kernels_in(data) == set() and cm.kernels_in(data) == {("convolve_rows_kernel", (1,))}


def test_the_library_holds_exactly_the_declared_kernels(lib):
    with open(capi.LIBRARY_PATH, "rb") as f:
        data = f.read()
    found = sm.kernels_in(data)
    declared = {(c.kernel, c.args) for c in sm.cells()}
    assert len(sm.cells()) == len(declared) == 5
    missing, surplus = sorted(declared - found), sorted(found - declared)
    print("declared and not in the library (%d):" % len(missing), missing)
    print("in the library and not declared (%d):" % len(surplus), surplus)
    assert not missing and not surplus


def test_every_named_case_exists_in_the_gpu_file():
    import test_gpu_convolve_stats as gpu
    assert gpu.__file__.endswith(sm.GPU_FILE)
    assert any(m.name == "gpu" for m in (gpu.pytestmark if isinstance(gpu.pytestmark, list) else [gpu.pytestmark]))
    for c in sm.cells():
        assert callable(getattr(gpu, c.case, None)) and c.case.startswith("test_"), c
