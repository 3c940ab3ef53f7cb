"""Kernel names out of a library's bytes, for the two census tests (test_window_kernel_census.py, test_encode_kernel_census.py).
The host object keeps every kernel's mangled name as a string (the runtime registers the kernel under it), so the names are read
from the bytes - names only, no code - and the template arguments from their Li<n>E / Lin<n>E (a negative int) / Lb<0|1>E groups.

TEST INFRASTRUCTURE (tests/ only).  Imports neither torch nor the library."""
import re

# _ZN3aad <length> <name> [I <arguments> E] E <parameter types>: a kernel of namespace aad, a template's instantiation or a plain
# function.  A name starts with a letter, so a __device_stub__ twin - its length prefix stands before "__device_stub__" - never matches.
NAME = re.compile(rb"_ZN3aad(\d+)([a-z][a-z0-9_]*_kernel)(?:I((?:L[ib]n?\d+E)+)E)?E")
ARG = re.compile(rb"L([ib])(n?)(\d+)E")


def kernels_in(data, keep=lambda name: True):
    """bytes -> the set of (kernel, template arguments) among the mangled names in them; keep(name) picks the kernels"""
    found = set()
    for m in NAME.finditer(data):
        name = m.group(2)
        if int(m.group(1)) != len(name):  # a wrong length prefix: no name of ours
            continue
        if not keep(name.decode()):
            continue
        args = tuple(-int(v) if neg else int(v) for _, neg, v in ARG.findall(m.group(3) or b""))
        found.add((name.decode(), args))
    return found


def is_window_kernel(name):
    return name.startswith("decode_window")
