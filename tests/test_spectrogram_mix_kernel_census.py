"""The census of the spectrogram stage's mix kernels: the instantiations of namespace aad::spectrum_mix that the built library
holds against the records of tests/spectrogram_mix_matrix.py.  The names are read from the library's bytes as
tests/kernel_names.py reads them - names only, no code - with a pattern for the nested namespace.  The two sets must be EQUAL, two
kernels, and every record names a case of tests/test_gpu_spectrogram_mix.py.  The older census tests' patterns - namespace aad
alone, aad::convolve, aad::spectrum - see none of them.  No GPU."""
import pytest

import aad_amd
import convolve_matrix
import kernel_names
import spectrogram_matrix as sm
import spectrogram_mix_matrix as mm
from aad_amd import capi


@pytest.fixture(scope="module")
def lib():
    return aad_amd.load_library()


def test_the_parser_on_names_written_by_hand():
    data = (b"\0_ZN3aad12spectrum_mix24spectrum_mix_rows_kernelILb1EEEvNS0_4ArgsE\0"
            b"_ZN3aad12spectrum_mix39__device_stub__spectrum_mix_rows_kernelILb0EEEvNS0_4ArgsE\0"
            b"_ZN3aad12spectrum_mix25spectrum_mix_rows_kernelILb0EEEvNS0_4ArgsE\0"  # a wrong length: no name of ours
            b"_ZN3aad8spectrum20spectrum_rows_kernelILb0EEEvNS0_4ArgsE\0"
            b"_ZN3aad24spectrum_mix_rows_kernelILb0EEEvNS_4ArgsE\0")                # namespace aad alone: not this family
    assert mm.kernels_in(data) == {("spectrum_mix_rows_kernel", (1,))}
    assert sm.kernels_in(data) == {("spectrum_rows_kernel", (0,))}
    assert kernel_names.kernels_in(data) == {("spectrum_mix_rows_kernel", (0,))}
    assert convolve_matrix.kernels_in(data) == set()


def test_the_library_holds_exactly_the_declared_kernels(lib):
    with open(capi.LIBRARY_PATH, "rb") as f:
        data = f.read()
    found = mm.kernels_in(data)
    declared = {(c.kernel, c.args) for c in mm.cells()}
    assert len(mm.cells()) == len(declared) == 2
    missing, surplus = sorted(declared - found), sorted(found - declared)
    print("declared and not in the library (%d):" % len(missing), missing)
    print("in the library and not declared (%d):" % len(surplus), surplus)
    assert not missing and not surplus
    for older in (kernel_names, convolve_matrix, sm):
        assert not any(name.startswith("spectrum_mix") for name, _ in older.kernels_in(data)), older.__name__
    assert len(sm.kernels_in(data)) == 2  # aad::spectrum keeps exactly its own two


def test_every_named_case_exists_in_the_gpu_file():
    import test_gpu_spectrogram_mix as gpu
    assert gpu.__file__.endswith(mm.GPU_FILE)
    assert any(m.name == "gpu" for m in (gpu.pytestmark if isinstance(gpu.pytestmark, list) else [gpu.pytestmark]))
    for c in mm.cells():
        assert callable(getattr(gpu, c.case, None)) and c.case.startswith("test_"), c
