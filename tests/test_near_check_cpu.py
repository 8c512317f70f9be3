"""service.check_near, the one host-side checker of a near ask's parameters, against the two it replaced
(check_near_params for the bounded form, check_near_wide_params for the wide one): tests/golden/near_check_verdicts.json
holds what those two returned or raised, recorded from them before they went, over a grid of good and bad values - each
bin limit itself and one bin past it, NaN and +-inf for eps and max_offset, every integer parameter at and past its
ends.  The unified checker must accept and refuse exactly as they did, with the same values and exception classes."""
import json
import os

import pytest

from tvidz_amd import corpus as tc, service

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "near_check_verdicts.json")
FORMS = {f.stem: f for f in service.NEAR_FORMS.values()}


def _dec(v):
    return float(v) if isinstance(v, str) else v                     # 'nan', 'inf', '-inf'


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")       # 2 x 1e308 bins: refused, as before
def test_check_near_accepts_and_refuses_as_the_two_checkers_it_replaced():
    cases = _cases()
    seen = set()
    for stem, args, verdict in cases:
        form, args = FORMS[stem], [_dec(a) for a in args]
        try:
            got = service.check_near(form, *args)
        except Exception as e:  # noqa: BLE001 - the class is what is compared
            got = type(e).__name__
        else:
            assert len(got) == 6 and [type(v) for v in got] == [float, float, int, int, int, int], (stem, args, got)
            got = list(got)
        want = verdict if isinstance(verdict, str) else [_dec(v) for v in verdict]
        assert got == want, (stem, args, got, want)
        seen.add((stem, "ok" if isinstance(verdict, list) else verdict))
    assert seen == {("align_topk", "ok"), ("align_topk", "ValueError"), ("align_topk", "TypeError"),
                    ("align_wide_topk", "ok"), ("align_wide_topk", "ValueError")}


def test_the_recorded_grid_holds_each_limit_and_one_past_it():
    """What the file must hold for the comparison above to mean something: each form's bin limit accepted and the next
    bin refused, NaN and inf for eps and max_offset refused, max_offset=None the widest of the wide form only, the
    flags 0 for the form without them."""
    verdicts = {(stem, tuple(map(str, args))): v for stem, args, v in _cases()}
    B = tc.ALIGN_WIDE_MAX_B

    def v(stem, eps, max_offset, k=4, min_votes=1, min_score=0, contain=False):
        return verdicts[(stem, tuple(map(str, (eps, max_offset, k, min_votes, min_score, contain))))]

    assert service.NEAR_MAX_BINS == 4096 and v("align_topk", 1.0, 2047.0) == [1.0, 2047.0, 4, 1, 0, 0]
    assert v("align_topk", 1.0, 2048.0) == "ValueError" and v("align_topk", 1.0, 2047.5) == "ValueError"
    assert v("align_wide_topk", 1.0, float(B)) == [1.0, float(B), 4, 1, 0, 0]
    assert v("align_wide_topk", 1.0, float(B + 1)) == "ValueError" and v("align_wide_topk", 1.0, B + 0.5) == "ValueError"
    assert v("align_wide_topk", 1.0, 2048.0) == [1.0, 2048.0, 4, 1, 0, 0]            # past the bounded limit: wide takes it
    for stem in FORMS:
        for bad in ("nan", "inf"):
            assert v(stem, bad, 3.0) == "ValueError" and v(stem, 1.0, bad) == "ValueError"
        assert v(stem, 1.0 / 30, 3.0, k=65) == "ValueError" and v(stem, 1.0 / 30, 3.0, k=64)[2] == 64
    assert v("align_topk", 1.0, None) == "TypeError"                                 # the widest is the wide form's
    assert v("align_wide_topk", 1.0, None, contain=True) == [1.0, float(B), 4, 1, 0, tc.ALIGN_CONTAIN]
