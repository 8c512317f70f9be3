"""The gfx950 code object of tvz_align_topk_merge, read without a GPU with the metadata readers of
tests/test_codeobj_cpu.py: the merge kernel is there once, under a name of its own, with no scratch, no spilled
registers and no LDS - it keeps a query's k rows in one wave's registers and never meets a barrier."""
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)

MERGE = "_ZN12_GLOBAL__N_126ts_align_topk_merge_kernelE"


def test_the_merge_kernel_exists_once(kernels):  # noqa: F811
    named = [n for n in kernels if n.startswith(MERGE)]
    assert len(named) == 1, sorted(n for n in kernels if "align" in n)     # n_lists and k are run-time arguments
    # the sweep's and the selection's kernels are still there, each once
    for other in ("20ts_align_topk_kernelE", "27ts_align_topk_reduce_kernelE", "15ts_align_kernelE"):
        assert len([n for n in kernels if other in n]) == 1, other


def test_no_scratch_no_spills_no_lds(kernels):  # noqa: F811
    (k,) = [k for n, k in kernels.items() if n.startswith(MERGE)]
    assert k[".private_segment_fixed_size"] == 0, k[".private_segment_fixed_size"]
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k
    assert k[".group_segment_fixed_size"] == 0, k[".group_segment_fixed_size"]
    # 256-thread blocks, a wave per query.  Reported: 44 VGPRs (four lists' 16-byte rows in flight + the kept pair)
    # -> eight waves per SIMD
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]
    assert k[".max_flat_workgroup_size"] == 256
