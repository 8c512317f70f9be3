"""The gfx950 code objects of tvz_align_topk, read without a GPU with the metadata readers of
tests/test_codeobj_cpu.py: both kernels under names of their own, no scratch, no spills, and the registers and
static LDS the launch assumes.  The figures are the compiler's resource report of the built kernels, with the
occupancy they buy written next to them."""
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)

# exclusion, thresholds, k and the bin count are run-time arguments: ONE instantiation each
SWEEP = "_ZN12_GLOBAL__N_120ts_align_topk_kernelE"
REDUCE = "_ZN12_GLOBAL__N_127ts_align_topk_reduce_kernelE"


def _named(kernels, prefix):  # noqa: F811
    return {n: k for n, k in kernels.items() if n.startswith(prefix)}


def test_both_kernels_exist_once_under_names_of_their_own(kernels):  # noqa: F811
    assert len(_named(kernels, SWEEP)) == 1, sorted(n for n in kernels if "align" in n)
    assert len(_named(kernels, REDUCE)) == 1, sorted(n for n in kernels if "align" in n)
    # tvz_align's own kernel is still there, and is neither of them
    old = [n for n in kernels if "ts_align_kernel" in n]
    assert len(old) == 1 and old[0] not in _named(kernels, SWEEP) and old[0] not in _named(kernels, REDUCE)


def test_no_scratch_and_no_spills(kernels):  # noqa: F811
    for prefix in (SWEEP, REDUCE):
        for n, k in _named(kernels, prefix).items():
            assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
            assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k)


def test_the_sweeps_registers_and_lds(kernels):  # noqa: F811
    (_, k), = _named(kernels, SWEEP).items()
    # 256-thread blocks, one wave per SIMD and block.  Reported: 63 VGPRs -> allocated 64 -> eight waves per SIMD, so
    # the LDS sets the occupancy: static 4,112 B (the four waves' lists, 64 x 16 B each, for the merge at the block's
    # end + the hit counter) + dynamic 8 B per query value + per wave 6 B per bin.  The inspector's defaults (200
    # values, 1,801 bins): 1,600 + 4 x 10,816 + 4,112 = 48,976 B -> three blocks = twelve waves per CU; the largest
    # call (4,095 values, 4,095 bins): 32,760 + 98,320 + 4,112 = 135,192 B -> one block, under a workgroup's 160 KiB.
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]
    assert 4 * 64 * 16 <= k[".group_segment_fixed_size"] <= 4 * 64 * 16 + 64, k[".group_segment_fixed_size"]
    assert k[".max_flat_workgroup_size"] == 256


def test_the_selection_kernel_fits_its_1024_thread_block(kernels):  # noqa: F811
    (_, k), = _named(kernels, REDUCE).items()
    # sixteen waves = four per SIMD: needs <= 128 VGPRs (reported: 40); LDS = sixteen waves' lists of 64 x 16 B
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]
    assert 16 * 64 * 16 <= k[".group_segment_fixed_size"] <= 16 * 64 * 16 + 64, k[".group_segment_fixed_size"]
    assert k[".max_flat_workgroup_size"] == 1024
