"""The tolerant match's gfx950 code objects, read without a GPU (the metadata readers of tests/test_codeobj_cpu.py):
no scratch, and the register budget their launch shapes assume - the sweep runs 256-thread blocks with up to 96 KiB
of LDS and wants eight waves per SIMD when its LDS table is small (at most 64 VGPRs)."""
import pytest

from tests.test_codeobj_cpu import kernels  # noqa: F401  (the module-scoped fixture)

TOL = ("ts_match_tol_kernel", "ts_tol_sort_kernel", "ts_tol_kth_fixup_kernel")


def test_tolerant_kernels_use_no_scratch(kernels):  # noqa: F811
    seen = {}
    for name, k in kernels.items():
        for t in TOL:
            if t in name:
                seen[t] = seen.get(t, 0) + 1
                assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
                assert k.get(".vgpr_spill_count", 0) == 0, (name, k)
    # the sweep: {M2, Top5, Count} x {pinned host hits, device hit lists} x {LDS table, device-memory table}
    assert seen == {"ts_match_tol_kernel": 12, "ts_tol_sort_kernel": 1, "ts_tol_kth_fixup_kernel": 1}, seen


def test_tolerant_sweep_fits_eight_waves_per_simd(kernels):  # noqa: F811
    n = 0
    for name, k in kernels.items():
        if "ts_match_tol_kernel" in name:
            n += 1
            assert k[".vgpr_count"] <= 64, (name, k[".vgpr_count"])
            # static LDS: the per-block hit staging of the device-list form (256 hits x 12 B) + a few words
            assert k[".group_segment_fixed_size"] <= 256 * 12 + 64, (name, k[".group_segment_fixed_size"])
    assert n == 12


@pytest.mark.parametrize("name", ["ts_tol_sort_kernel", "ts_tol_kth_fixup_kernel"])
def test_helpers_stay_small(kernels, name):  # noqa: F811
    k = [v for n, v in kernels.items() if name in n]
    assert len(k) == 1 and k[0][".vgpr_count"] <= 64
