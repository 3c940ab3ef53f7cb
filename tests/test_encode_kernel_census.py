"""The census of every kernel but the window decoders: the instantiations the built library holds against the case table of
tests/encode_matrix.py (the window decoders: test_window_kernel_census.py against tests/window_matrix.py).  The names come from
the library's bytes through tests/kernel_names.py - names only, no code.  The two sets must be EQUAL: a kernel without a record
has no case that runs it, a record without a kernel is a case that runs something else.  No GPU."""
import importlib
import os

import pytest

import aad_amd
import encode_matrix as em
import kernel_names
from aad_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    return aad_amd.load_library()


def kernels_in(data):
    return kernel_names.kernels_in(data, lambda name: not kernel_names.is_window_kernel(name))


def test_the_parser_on_names_written_by_hand():
    data = (b"\0_ZN3aad21encode_streams_kernelILi3ELi2ELb1ELb0ELb1ELb0ELb0ELb1ELi2ELi4EEEvNSt11conditionalIXeqT8_LNS_9RecOutputE0EE\0"
            b"_ZN3aad36__device_stub__encode_streams_kernelILi4ELi1ELb0ELb0ELb0ELb0ELb0ELb0ELi0ELi0EEEvNS_10EncodeArgsE\0"  # a stub twin
            b"_ZN3aad22encode_streams_kernelILi2ELi1ELb0ELb0ELb0ELb0ELb0ELb0ELi0ELi0EEEvNS_10EncodeArgsE\0"  # a wrong length: no name of ours
            b"_ZN3aad26resample_rows_stats_kernelILin1EEEvNS_15ResampleMixArgsE\0"                             # a negative argument
            b"_ZN3aad23compare_segments_kernelENS_11CompareArgsE\0"                                            # no template
            b"_ZN3aad38__device_stub__compare_segments_kernelENS_11CompareArgsE\0"
            b"_ZN3aad20decode_window_kernelILi4ELi1ELb0ELi0EEEvNS_10WindowArgsE\0"                             # the other census' kernel
            b"_ZN3aad19decode_tiled_kernelILi4ELi2ELb1EEEvNS_10DecodeArgsE\0")
    assert kernels_in(data) == {("encode_streams_kernel", (3, 2, 1, 0, 1, 0, 0, 1, 2, 4)), ("resample_rows_stats_kernel", (-1,)),
                                ("compare_segments_kernel", ()), ("decode_tiled_kernel", (4, 2, 1))}
    assert kernel_names.kernels_in(data, kernel_names.is_window_kernel) == {("decode_window_kernel", (4, 1, 0, 0))}


def test_the_table_follows_the_holes_of_the_dispatch():
    """the shape of the table, as the dispatch code states it - counted on the table alone"""
    enc = [c.args for c in em.cells() if c.kernel == "encode_streams_kernel"]
    for bits, chf, ms, quad, trials, dual, ring, seg, inp, rec in enc:
        assert not (inp == em.IN_PLANAR_I16 and chf == 1)                         # mono int16 rows are the interleaved layout
        assert not (inp == em.IN_INTERLEAVED and rec != em.REC_NONE and chf != 1)  # an interleaved REC kernel for mono alone
        assert not (rec != em.REC_NONE and (dual or ring))                        # no DUAL and no RING with a REC
        assert not (ring and seg)                                                 # no RING with SEG
        assert not (chf == 0 and (quad or ring or dual))                          # CHF = 0 on the dense, ring-free kernels only
        assert not (dual and not (quad and trials)) and not (ring and (quad or trials)) and not (ms and chf != 2)
    assert len(em.ENCODE_PAIRS) == 18 and len(em.encode_groups()) == 108
    nt = [c.args for c in em.cells() if c.kernel == "decode_blocks_kernel" and c.args[4]]
    assert sorted(nt) == [(2, 2, 0, 0, 1), (2, 2, 1, 0, 1), (4, 2, 0, 0, 1), (4, 2, 1, 0, 1)]  # streamed stores: dense stereo, 4 and 2 bits


def test_the_library_holds_exactly_the_declared_kernels(lib):
    with open(capi.LIBRARY_PATH, "rb") as f:
        found = kernels_in(f.read())
    declared = {(c.kernel, c.args) for c in em.cells()}
    assert not set(em.UNREACHABLE) & declared, "a kernel is either reached or unreachable"
    expected = declared | set(em.UNREACHABLE)
    missing, surplus = sorted(expected - found), sorted(found - expected)
    print("declared and not in the library (%d):" % len(missing), missing)
    print("in the library and not declared (%d):" % len(surplus), surplus)
    assert not missing and not surplus, ("declared, not built", missing[:8], "built, no case", surplus[:8])
    by_kernel = {}
    for kernel, _ in declared:
        by_kernel[kernel] = by_kernel.get(kernel, 0) + 1
    print("reachable kernels per family:", by_kernel, "total", len(declared), "unreachable", len(em.UNREACHABLE))
    assert by_kernel == em.COUNTS
    assert by_kernel["encode_streams_kernel"] == 1140 and len(declared) == 1244 and len(found) == 1244 + len(em.UNREACHABLE)


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


def _has_gpu_mark(module):
    marks = getattr(module, "pytestmark", [])
    return any(m.name == "gpu" for m in (marks if isinstance(marks, list) else [marks]))


def test_every_named_case_exists_in_the_gpu_file():
    import test_gpu_encode_matrix as gpu
    assert gpu.__file__.endswith(em.GPU_FILE) and _has_gpu_mark(gpu)
    named = {c.case for c in em.matrix_cells()}
    have = _case_ids(gpu)
    assert named <= have, sorted(named - have)
    assert len(named) == len(em.encode_groups()) + len(em.decode_groups()) == 117


def test_every_named_existing_test_exists_and_needs_a_gpu():
    for c in em.other_cells():
        file, _, function = c.case.partition("::")
        assert file.startswith("test_gpu_") and os.path.exists(os.path.join(HERE, file)), c
        module = importlib.import_module(file[:-3])
        fn = getattr(module, function, None)
        assert callable(fn), c
        assert _has_gpu_mark(module) or any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), c
