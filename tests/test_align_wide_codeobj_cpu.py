"""The gfx950 code objects of tvz_align_wide_topk, read without a GPU with the metadata readers of
tests/test_codeobj_cpu.py: the windowed sweep and its selection once each under names of their own, no scratch, no
spills, the registers and static LDS the launch assumes - and both new exports, with the binding's table matching."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)
from tvidz_amd import _lib, build as tbuild

# exclusion, thresholds, flags, k, the bin count and the window width are run-time arguments: ONE instantiation each
SWEEP = "_ZN12_GLOBAL__N_122ts_alignw_sweep_kernelE"
REDUCE = "_ZN12_GLOBAL__N_123ts_alignw_reduce_kernelE"
EXPORTS = ("tvz_align_wide_topk", "tvz_align_wide_topk_workspace_bytes")


def _named(kernels, prefix):  # noqa: F811
    return {n: k for n, k in kernels.items() if n.startswith(prefix)}


def test_both_kernels_exist_once_under_names_of_their_own(kernels):  # noqa: F811
    assert len(_named(kernels, SWEEP)) == 1, sorted(n for n in kernels if "align" in n)
    assert len(_named(kernels, REDUCE)) == 1, sorted(n for n in kernels if "align" in n)
    for n in list(_named(kernels, SWEEP)) + list(_named(kernels, REDUCE)):
        # the bounded search's kernels are pinned by name in tests/test_align_topk_codeobj_cpu.py: these are neither
        assert "ts_align_kernel" not in n and "ts_align_topk_kernel" not in n and "ts_align_topk_reduce_kernel" not in n
    assert len([n for n in kernels if "ts_align_topk_kernel" in n]) == 1


def test_no_scratch_and_no_spills(kernels):  # noqa: F811
    for prefix in (SWEEP, REDUCE):
        for n, k in _named(kernels, prefix).items():
            assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
            assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k)


def test_the_sweeps_registers_and_lds(kernels):  # noqa: F811
    (_, k), = _named(kernels, SWEEP).items()
    # 256-thread blocks, one wave per SIMD and block.  Reported: 70 VGPRs -> allocated 72 -> seven waves per SIMD, so
    # the LDS sets the occupancy for every call of more than ~600 bins: static 5,136 B (the four waves' lists, 64 x 20 B
    # each, for the merge at the block's end + the hit counter) + dynamic 8 B per query value + per wave 6 B per bin
    # of a window and the touched count.  B <= 2047 is one window of all bins, the bounded sweep's dynamic LDS: 200
    # values at B = 900 (1,802 bins): 1,600 + 4 x 10,816 + 5,136 = 50,000 B -> three blocks = twelve waves per CU;
    # 4,095 values at B = 2047: 32,760 + 98,320 + 5,136 = 136,216 B, the largest call, under a workgroup's 160 KiB
    # (163,840 B).  Beyond, windows of 1,024 bins + 1,024 B of resume positions per wave: 200 values -> 1,600 +
    # 4 x 7,172 + 5,136 = 35,424 B -> four blocks = sixteen waves per CU; 4,095 values -> 66,584 B -> two blocks.
    assert k[".vgpr_count"] <= 72, k[".vgpr_count"]
    assert 4 * 64 * 20 <= k[".group_segment_fixed_size"] <= 4 * 64 * 20 + 64, k[".group_segment_fixed_size"]
    assert k[".group_segment_fixed_size"] + 4095 * 8 + 4 * (4096 * 6 + 4) <= 160 * 1024
    assert k[".group_segment_fixed_size"] + 4095 * 8 + 4 * (1024 * 6 + 4 + 512 * 2) <= 160 * 1024 // 2
    assert k[".max_flat_workgroup_size"] == 256


def test_the_selection_kernel_fits_its_1024_thread_block(kernels):  # noqa: F811
    (_, k), = _named(kernels, REDUCE).items()
    # sixteen waves = four per SIMD: needs <= 128 VGPRs (reported: 49); LDS = sixteen waves' lists of 64 x 20 B
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]
    assert 16 * 64 * 20 <= k[".group_segment_fixed_size"] <= 16 * 64 * 20 + 64, k[".group_segment_fixed_size"]
    assert k[".max_flat_workgroup_size"] == 1024


def test_both_exports_are_in_the_library_and_in_the_binding():
    if not os.path.exists(tbuild.SO):
        pytest.skip("libtvz.so is not built")
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        defined = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tbuild.SO], text=True).splitlines()
                   if ln.strip()}
        assert set(EXPORTS) <= defined, sorted(set(EXPORTS) - defined)
    lib = C.CDLL(tbuild.SO)
    for name in EXPORTS:
        assert getattr(lib, name) is not None
    # the binding's table: the header's argument list, type by type
    res, args = _lib.SIGNATURES["tvz_align_wide_topk"]
    P = C.c_void_p
    assert res is C.c_int
    assert args == [P, P, P, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_uint32, P, C.c_int32,
                    P, P, C.c_size_t, P]
    res, args = _lib.SIGNATURES["tvz_align_wide_topk_workspace_bytes"]
    assert res is C.c_size_t and args == [C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    # ... and the same sizing rule as the bounded call, at 20 bytes per kept hit instead of 16
    lib.tvz_align_wide_topk_workspace_bytes.restype = C.c_size_t
    lib.tvz_align_wide_topk_workspace_bytes.argtypes = args
    lib.tvz_align_topk_workspace_bytes.restype = C.c_size_t
    lib.tvz_align_topk_workspace_bytes.argtypes = args
    for Q, L, keys, k in ((1, 200, 0, 16), (16, 4095, 0, 64), (70, 40, 1234, 1), (1, 0, 0, 1)):
        wide, old = lib.tvz_align_wide_topk_workspace_bytes(Q, L, keys, k), lib.tvz_align_topk_workspace_bytes(Q, L, keys, k)
        lists = max(6080, 95 * Q) * k
        assert old < wide <= old + lists * 4 + 256, (Q, L, keys, k, wide, old)
    assert lib.tvz_align_wide_topk_workspace_bytes(1, 10, 0, 0) == 0 == lib.tvz_align_wide_topk_workspace_bytes(-1, 10, 0, 1)

