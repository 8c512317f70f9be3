"""The gfx950 code object of tvz_align_wide_topk_merge, read without a GPU with the metadata readers of
tests/test_codeobj_cpu.py: the wide merge kernel is there once, under a name of its own, with no scratch, no spilled
registers and no LDS - as the bounded merge, it keeps a query's k rows in one wave's registers and never meets a
barrier.  And the four new exports: defined in the library, the binding's table matching the header type by type, the
sharded sizing function equal to the plain wide one plus the blocks."""
import ctypes as C
import os
import re
import shutil
import subprocess

from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tvidz_amd import _lib, build as tbuild

MERGE = "_ZN12_GLOBAL__N_122ts_alignw_merge_kernelE"
BOUNDED = "_ZN12_GLOBAL__N_126ts_align_topk_merge_kernelE"
EXPORTS = ("tvz_align_wide_topk_merge", "tvz_align_wide_topk_shards", "tvz_align_wide_topk_sharded_workspace_bytes",
           "tvz_align_wide_topk_sharded")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tvz.h")


def test_the_wide_merge_kernel_exists_once_under_its_own_name(kernels):  # noqa: F811
    named = [n for n in kernels if n.startswith(MERGE)]
    assert len(named) == 1, sorted(n for n in kernels if "align" in n)     # n_lists, k and the flags are run-time arguments
    # the bounded merge is still a kernel of its own (tests/test_align_topk_sharded_codeobj_cpu.py pins it by name)
    assert len([n for n in kernels if n.startswith(BOUNDED)]) == 1 and not named[0].startswith(BOUNDED)
    # ... and the sweep's and the selection's kernels of the wide call are there, each once
    for other in ("22ts_alignw_sweep_kernelE", "23ts_alignw_reduce_kernelE"):
        assert len([n for n in kernels if other in n]) == 1, other


def test_no_scratch_no_spills_no_lds(kernels):  # noqa: F811
    (k,) = [k for n, k in kernels.items() if n.startswith(MERGE)]
    assert k[".private_segment_fixed_size"] == 0, k[".private_segment_fixed_size"]
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k
    assert k[".group_segment_fixed_size"] == 0, k[".group_segment_fixed_size"]
    # 256-thread blocks, a wave per query.  Reported: 46 VGPRs (four lists' 16-byte rows in flight + the kept
    # hit's two words and votes) -> eight waves per SIMD, the bounded merge's own cap
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]
    assert k[".max_flat_workgroup_size"] == 256


def _ctype(decl):
    """One parameter (or result) of a header prototype -> the ctypes type the binding's table names for it."""
    decl = decl.strip()
    if "*" in decl:
        return C.c_void_p
    base = re.sub(r"\bconst\b", "", decl).split()[0]
    return {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double,
            "size_t": C.c_size_t}[base]


def _prototype(text, name):
    m = re.search(r"^(\w+)\s+" + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, name
    return _ctype(m.group(1)), [_ctype(p) for p in m.group(2).split(",")]


def test_the_four_exports_are_in_the_library_and_match_the_header():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
               if ln.strip()}
    assert set(EXPORTS) <= defined, sorted(set(EXPORTS) - defined)
    text = open(HEADER).read()
    for name in EXPORTS:
        res, args = _prototype(text, name)
        assert _lib.SIGNATURES[name] == (res, args), (name, _lib.SIGNATURES[name], res, args)
    # (the reader reads what it should: the bounded forms and the plain wide call come out as the table has them)
    for name in ("tvz_align_topk_merge", "tvz_align_topk_sharded", "tvz_align_wide_topk"):
        assert _lib.SIGNATURES[name] == _prototype(text, name), name
    # the wide forms are the bounded ones with the flags: one uint32 more, where the header puts it
    P = C.c_void_p
    assert _lib.SIGNATURES["tvz_align_wide_topk_merge"][1] == [P, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, P, P, P, P, P]
    for wide, bounded in (("tvz_align_wide_topk_shards", "tvz_align_topk_shards"),
                          ("tvz_align_wide_topk_sharded", "tvz_align_topk_sharded")):
        w, b = _lib.SIGNATURES[wide][1], _lib.SIGNATURES[bounded][1]
        assert len(w) == len(b) + 1 and [t for t in w if t is not C.c_uint32] == b and w.count(C.c_uint32) == 1
    assert _lib.VERSION == 404 and _lib.load().tvz_version() == 404            # new exports only


def test_the_sharded_sizing_is_the_plain_wide_sizing_plus_the_blocks():
    lib = _lib.load()
    for Q, L, keys, k in ((1, 200, 0, 16), (16, 4095, 0, 64), (70, 40, 1234, 1), (1, 0, 0, 1), (0, 10, 0, 4), (64, 40, 0, 16)):
        plain = lib.tvz_align_wide_topk_workspace_bytes(Q, L, keys, k)
        for n in (-3, 0, 1, 2, 8, 16):
            size = lib.tvz_align_wide_topk_sharded_workspace_bytes(Q, L, keys, k, n)
            blocks = (1 + max(n, 1)) * Q * (k + 1) * 16
            # two more parts, each rounded up to 256 B
            assert plain + blocks <= size <= plain + blocks + 2 * 256, (Q, L, keys, k, n, size, plain)
    assert lib.tvz_align_wide_topk_sharded_workspace_bytes(1, 10, 0, 0, 1) == 0
    assert lib.tvz_align_wide_topk_sharded_workspace_bytes(-1, 10, 0, 1, 1) == 0
