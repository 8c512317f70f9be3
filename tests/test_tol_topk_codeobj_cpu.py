"""The gfx950 code objects of the tolerant top-k form (tvz_match_tol_topk), read without a GPU with the metadata
readers of tests/test_codeobj_cpu.py: the expected instantiations under names of their own, no scratch, no spills,
and the registers and static LDS the launch shape assumes.  The figures are the compiler's resource report of the
built kernels, with the occupancy they buy written next to them."""
from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)

SWEEP, REDUCE = "ts_tol_topk_kernel", "ts_tol_topk_reduce_kernel"
WAVE_LISTS = 64 * 8 * 2                    # per wave: its kept list + its stage, 64 words of 8 B each


def _named(kernels, name):  # noqa: F811
    return {n: k for n, k in kernels.items() if name in n}


def test_the_new_kernels_exist_under_names_of_their_own(kernels):  # noqa: F811
    # the sweep: kModeM2 and kModeTop5, the sorted query always in LDS (no device-memory table form, no count-only
    # form, no pinned-host form); one selection kernel
    assert len(_named(kernels, SWEEP)) == 2, sorted(_named(kernels, SWEEP))
    assert len(_named(kernels, REDUCE)) == 1
    # ... and none of them is counted among the list form's code objects (tests/test_tol_codeobj_cpu.py)
    for n in list(_named(kernels, SWEEP)) + list(_named(kernels, REDUCE)):
        assert not any(old in n for old in ("ts_match_tol_kernel", "ts_tol_sort_kernel", "ts_tol_kth_fixup_kernel")), n


def test_no_scratch_and_no_spills(kernels):  # noqa: F811
    for name in (SWEEP, REDUCE):
        assert _named(kernels, name), name
        for n, k in _named(kernels, name).items():
            assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
            assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k)


def test_the_sweeps_registers_and_lds_are_what_its_launch_assumes(kernels):  # noqa: F811
    sweeps = sorted(_named(kernels, SWEEP).items())          # ILi0E = kModeM2, ILi1E = kModeTop5
    (_, m2), (_, top5) = sweeps
    # 256-thread blocks: one wave per SIMD and block.  gfx950 hands a wave its VGPRs in steps of 8 out of 512 per
    # SIMD lane: <= 64 keeps the eight waves per SIMD the list form has (the compiler reports 62 for kModeM2);
    # the five-position form carries its five positions per lane through the row (reported: 65, allocated 72)
    # and runs seven.  Either way a 200-timestamp query's 6.4 KiB of LDS per block allows 24 blocks per CU, so the
    # registers, not the LDS, set the occupancy there; a 4,095-timestamp query (52 KiB per block) allows three.
    assert m2[".vgpr_count"] <= 64, m2[".vgpr_count"]
    assert top5[".vgpr_count"] <= 72, top5[".vgpr_count"]
    for k in (m2, top5):
        # static LDS: four waves' lists and stages + the block's hit counter; the launch adds the sorted query
        # (tol_lds_bytes, at most 48 KiB) and checks the sum against a workgroup's 160 KiB with this bound
        assert 4 * WAVE_LISTS <= k[".group_segment_fixed_size"] <= 4 * WAVE_LISTS + 64, k[".group_segment_fixed_size"]
        assert k[".max_flat_workgroup_size"] == 256


def test_the_selection_kernel_fits_its_1024_thread_block(kernels):  # noqa: F811
    (_, k), = _named(kernels, REDUCE).items()
    # sixteen waves = four per SIMD: needs <= 128 VGPRs (reported: 44); LDS = sixteen waves' lists and stages
    assert k[".vgpr_count"] <= 64, k[".vgpr_count"]
    assert 16 * WAVE_LISTS <= k[".group_segment_fixed_size"] <= 16 * WAVE_LISTS + 64
    assert k[".max_flat_workgroup_size"] == 1024
