#!/usr/bin/env python3
"""Two builds of libtvz.so, kernel by kernel, without a GPU: the gfx950 code objects' metadata notes (registers, LDS,
scratch, spills, arguments) and a hash of every kernel function's bytes.  Shows that a change left the existing
kernels as they were.
   python3 profiles/codeobj_compare.py PARENT/tvidz_amd/libtvz.so tvidz_amd/libtvz.so"""
import hashlib
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_codeobj_cpu import _code_objects, _kernel_metadata  # noqa: E402


def funcs(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    sh = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for s in sh:
        if s[1] != 2:
            continue
        stroff = sh[s[6]][4]
        for p in range(s[4], s[4] + s[5], 24):
            name, info, other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, p)
            if info & 0xF != 2 or not size:
                continue
            e = elf.index(b"\0", stroff + name)
            nm = elf[stroff + name:e].decode()
            sec = sh[shndx]
            o = sec[4] + value - sec[3]
            out[nm] = hashlib.sha1(elf[o:o + size]).hexdigest() + ":%d" % size
    return out


def load(path):
    md, tx = {}, {}
    for co in _code_objects(open(path, "rb").read()):
        for k in _kernel_metadata(co):
            md[k[".name"]] = k
        tx.update(funcs(co))
    return md, tx


a_md, a_tx = load(sys.argv[1])
b_md, b_tx = load(sys.argv[2])
print("kernels parent", len(a_md), "branch", len(b_md))
print("only in branch:", sorted(set(b_md) - set(a_md)))
print("only in parent:", sorted(set(a_md) - set(b_md)))
bad = 0
for n in sorted(set(a_md) & set(b_md)):
    if a_md[n] != b_md[n]:
        bad += 1
        print("METADATA DIFFERS", n, {k: (a_md[n].get(k), b_md[n].get(k)) for k in a_md[n] if a_md[n].get(k) != b_md[n].get(k)})
    if a_tx.get(n) != b_tx.get(n):
        bad += 1
        print("TEXT DIFFERS", n, a_tx.get(n), b_tx.get(n))
print("differences:", bad)
for n in sorted(set(b_md) - set(a_md)):
    k = b_md[n]
    print(n, {x: k.get(x) for x in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
                                    ".vgpr_spill_count", ".sgpr_spill_count", ".max_flat_workgroup_size")})
