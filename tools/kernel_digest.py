#!/usr/bin/env python3
"""kernel_digest.py LIBRARY - what the device side of a built libaad_hip.so consists of, as text that `diff` can compare.

For every gfx950 code object embedded in LIBRARY (llvm-objdump --offloading) one line per device function, with its size and a hash
of its bytes in .text, and one per kernel descriptor (<kernel>.kd in .rodata: registers, LDS, scratch), sorted by symbol:

    <first 16 hex digits of the bytes' sha256> <size> <section> <symbol>

Two builds whose digests are equal launch byte-identical device code, so a change that shows an empty diff against its parent
moved no kernel and can only differ from it on the host.  Host only; LLVM_BIN names the directory of llvm-objdump and
llvm-readelf (default: $ROCM_PATH/llvm/bin, /opt/rocm/llvm/bin)."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"))


def tool(name, *args, **kw):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True, **kw).stdout


def code_object_rows(path):
    """the digest lines of one extracted code object (an ELF for the GPU)"""
    with open(path, "rb") as f:
        blob = f.read()
    sections = {}  # index -> (name, address, file offset)
    for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", tool("llvm-readelf", "-S", "-W", path)):
        sections[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
    rows = []
    for line in tool("llvm-readelf", "-s", "-W", path).splitlines():
        f = line.split()  # Num: Value Size Type Bind Vis Ndx Name
        if len(f) < 8 or f[3] not in ("FUNC", "OBJECT") or not f[6].isdigit():
            continue
        value, size, index, symbol = int(f[1], 16), int(f[2]), int(f[6]), f[7]
        section, address, offset = sections.get(index, ("", 0, 0))
        if size == 0 or not (section == ".text" or (section == ".rodata" and symbol.endswith(".kd"))):
            continue
        data = blob[offset + value - address: offset + value - address + size]
        rows.append((symbol, "%s %7d %s %s" % (hashlib.sha256(data).hexdigest()[:16], size, section, symbol)))
    return rows


def main(library):
    tmp = tempfile.mkdtemp()
    try:
        local = os.path.join(tmp, "library.so")  # llvm-objdump writes the code objects next to its input
        shutil.copy(library, local)
        tool("llvm-objdump", "--offloading", local, cwd=tmp)
        rows = []
        for name in sorted(os.listdir(tmp)):
            if "gfx950" in name:
                rows += code_object_rows(os.path.join(tmp, name))
        if not rows:
            sys.exit("kernel_digest.py: no gfx950 code object in %s" % library)
        for _, row in sorted(rows):
            print(row)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
