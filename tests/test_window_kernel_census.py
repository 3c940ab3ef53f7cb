"""The census of window decode kernels: the instantiations the built library holds against the case table of
tests/window_matrix.py.  The host object keeps every kernel's mangled name as a string (the runtime registers the kernel under
it), so the names are read from the library's bytes - names only, no code - and the template arguments from their Li<n>E /
Lb<0|1>E groups.  The two sets must be EQUAL: a kernel without a record has no matrix case that runs it, a record without a kernel
is a case that runs something else.  No GPU."""
import pytest

import aad_amd
import kernel_names
import window_matrix as wm
from aad_amd import capi


@pytest.fixture(scope="module")
def lib():
    return aad_amd.load_library()


def kernels_in(data):
    """bytes -> the set of (kernel, template arguments) among the mangled names of window decode kernels in them (the parser:
    tests/kernel_names.py, shared with test_encode_kernel_census.py; a __device_stub__ twin and a wrong length prefix never match)"""
    return kernel_names.kernels_in(data, kernel_names.is_window_kernel)


def test_the_parser_on_names_written_by_hand():
    data = (b"\0_ZN3aad20decode_window_kernelILi4ELi1ELb0ELi0EEEvNS_10WindowArgsE\0"
            b"_ZN3aad35__device_stub__decode_window_kernelILi4ELi2ELb1ELi5EEEvNS_10WindowArgsE\0"
            b"_ZN3aad45decode_window_channel_mix_placed_stats_kernelILi2ELi2ELb1ELi1EEEvNS_31ChannelMixWindowPlacedStatsArgsE\0"
            b"_ZN3aad21decode_window_kernelILi3ELi1ELb0ELi0EEEvNS_10WindowArgsE\0")  # a wrong length: no name of ours
    assert kernels_in(data) == {("decode_window_kernel", (4, 1, 0, 0)),
                                ("decode_window_channel_mix_placed_stats_kernel", (2, 2, 1, 1))}


def test_the_library_holds_exactly_the_declared_kernels(lib):
    with open(capi.LIBRARY_PATH, "rb") as f:
        found = kernels_in(f.read())
    declared = {(c.kernel, c.args) for c in wm.cells()}
    assert not set(wm.UNREACHABLE) & declared, "a kernel is either reached or unreachable"
    expected = declared | set(wm.UNREACHABLE)
    missing, surplus = sorted(expected - found), sorted(found - expected)
    print("declared and not in the library (%d):" % len(missing), missing)
    print("in the library and not declared (%d):" % len(surplus), surplus)
    assert not missing and not surplus, ("declared, not built", missing[:8], "built, no matrix case", surplus[:8])
    per_unit = wm.cells_per_unit()
    print("kernels per unit:", per_unit, "total", len(found))
    by_kernel = {}
    for kernel, _ in found:
        by_kernel[kernel] = by_kernel.get(kernel, 0) + 1
    for unit, kernel, _, _ in wm.UNITS:
        assert by_kernel.pop(kernel) == per_unit[unit] + sum(k == kernel for k, _ in wm.UNREACHABLE), unit
    assert not by_kernel, by_kernel


def _case_ids(module):
    """the ids of the parametrised test cases of a module, from the parametrize marks on its test functions"""
    ids = set()
    for name, fn in vars(module).items():
        if not name.startswith("test_") or not callable(fn):
            continue
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        if not marks:
            ids.add(name)
        for m in marks:
            assert len(marks) == 1 and callable(m.kwargs.get("ids")), name
            ids |= {"%s[%s]" % (name, m.kwargs["ids"](v)) for v in m.args[1]}
    return ids


def test_every_named_case_exists_in_the_gpu_file():
    import test_gpu_window_decode_matrix as gpu
    assert gpu.__file__.endswith(wm.GPU_FILE)
    assert any(m.name == "gpu" for m in (gpu.pytestmark if isinstance(gpu.pytestmark, list) else [gpu.pytestmark]))
    named = {c.case for c in wm.cells()}
    have = _case_ids(gpu)
    assert named <= have, sorted(named - have)
    assert len(named) == len(wm.GEOMETRIES) + len(wm.MIXED_PLANS) + len(wm.OUT_CHANNELS)
