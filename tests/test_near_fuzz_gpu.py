"""A seeded, bounded slice of the near-duplicate differential (tests/near_fuzz_cases.py) inside the `-m gpu` suite:
random tables, uploads derived from them and random in-contract parameters through tvz_align_topk, tvz_align_wide_topk
(alone, TVZ_ALIGN_CONTAIN, TVZ_ALIGN_TWO_BINS), tvz_align_rates_topk, tvz_align_span_topk (alone, TVZ_ALIGN_LOCAL),
tvz_align_parts / tvz_align_parts_flags, tvz_align_candidates / tvz_align_candidates_rates, their _shards forms and the
device merges, against the plain references, whole blocks bit for bit, with upserts, build_index and the gap index
switched between the calls.

Each test runs a FIXED number of cases, so a seed always runs the same ones.  The count is the reference's own cost,
nothing the library does: the generator with the references alone (near_fuzz_cases.run(seed, CASES, device=None)) took,
on the CPU of the build machine and for 80 cases,
    seed 11: 4.8 s    seed 2024: 4.9 s    seed 31337: 6.4 s
(about 8 s is the bound; at 100 cases seed 31337 is past it), and the same slices with every call made on an MI355X
took 5.4 s, 6.8 s and 7.0 s.  The last test asserts that the three slices together reached every mechanism the counters
name; tests/test_near_fuzz_cases_cpu.py asserts the same of the references alone, so the condition holds before a
device is asked."""
import pytest

from tests import near_fuzz_cases as nf

pytestmark = pytest.mark.gpu
SEEDS = (11, 2024, 31337)
CASES = 80
_totals = {}


def reached(totals):
    """What the slices must have reached: every counter at least once, every form at least 5 times."""
    missing = [k for k, v in totals.items() if k not in ("calls", "seconds") and v < 1]
    missing += [f for f in nf.FORMS if totals["calls"].get(f, 0) < 5]
    return missing


@pytest.mark.parametrize("seed", SEEDS)
def test_near_fuzz_slice_against_the_references(seed):
    stats = nf.run(seed, CASES)
    assert stats["cases"] == CASES, stats
    nf.add_stats(_totals, stats)
    print(stats)


@pytest.mark.parametrize("name", ("b_fused_product", "f_parts_keep_votes", "g_unsorted_gap_codes"))
def test_the_comparison_on_the_device_bites(name):
    """The same walk with a perturbed reference of tests/test_near_fuzz_cases_cpu.py is a mismatch, named by seed, case,
    call and query: the comparison with the device's blocks is not vacuous.  (These three show within the first eight
    cases of the first seed; the CPU module shows all seven over the whole slice.)"""
    from tests.test_near_fuzz_cases_cpu import PERTURBED
    with pytest.raises(AssertionError, match="NEAR MISMATCH") as e:
        nf.run(SEEDS[0], 8, refs=nf.refs_with(**PERTURBED[name][0]))
    where = e.value.args[0][1]
    assert where["seed"] == SEEDS[0] and {"case", "call", "qi", "form"} <= set(where), where


def test_near_fuzz_slices_reached_every_mechanism():
    assert _totals.get("cases") == CASES * len(SEEDS), "the slices did not run"
    assert not reached(_totals), (reached(_totals), _totals)
