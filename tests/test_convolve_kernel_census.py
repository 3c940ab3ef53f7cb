"""The census of the convolve stage's kernels: the instantiations of namespace aad::convolve that the built library holds against
the records of tests/convolve_matrix.py.  The names are read from the library's bytes as tests/kernel_names.py reads them - names
only, no code - with a pattern for the nested namespace.  The two sets must be EQUAL, 1 + 4 + 6 kernels, and every record names a
case of tests/test_gpu_convolve.py.  The two older census tests read names of namespace aad alone and neither count nor miss
these.  No GPU."""
import pytest

import aad_amd
import convolve_matrix as cm
import kernel_names
from aad_amd import capi


@pytest.fixture(scope="module")
def lib():
    return aad_amd.load_library()


def test_the_parser_on_names_written_by_hand():
    data = (b"\0_ZN3aad8convolve23convolve_resolve_kernelENS0_11ResolveArgsE\0"
            b"_ZN3aad8convolve38__device_stub__convolve_resolve_kernelENS0_11ResolveArgsE\0"
            b"_ZN3aad8convolve25convolve_rows_gain_kernelILi4ELb1EEEvNS0_8GainArgsE\0"
            b"_ZN3aad8convolve21convolve_rows_kernelILi5EEEvNS0_8RowsArgsE\0"  # a wrong length: no name of ours
            b"_ZN3aad20convolve_rows_kernelILi1EEEvNS_8RowsArgsE\0")          # namespace aad alone: not this family
    assert cm.kernels_in(data) == {("convolve_resolve_kernel", ()), ("convolve_rows_gain_kernel", (4, 1))}
    # and the pattern of the older census tests sees none of the family
    assert kernel_names.kernels_in(data) == {("convolve_rows_kernel", (1,))}


def test_the_library_holds_exactly_the_declared_kernels(lib):
    with open(capi.LIBRARY_PATH, "rb") as f:
        data = f.read()
    found = cm.kernels_in(data)
    declared = {(c.kernel, c.args) for c in cm.cells()}
    assert len(cm.cells()) == len(declared) == 11
    missing, surplus = sorted(declared - found), sorted(found - declared)
    print("declared and not in the library (%d):" % len(missing), missing)
    print("in the library and not declared (%d):" % len(surplus), surplus)
    assert not missing and not surplus
    assert not any(name.startswith("convolve") for name, _ in kernel_names.kernels_in(data))


def test_every_named_case_exists_in_the_gpu_file():
    import test_gpu_convolve as gpu
    assert gpu.__file__.endswith(cm.GPU_FILE)
    assert any(m.name == "gpu" for m in (gpu.pytestmark if isinstance(gpu.pytestmark, list) else [gpu.pytestmark]))
    for c in cm.cells():
        assert callable(getattr(gpu, c.case, None)) and c.case.startswith("test_"), c
