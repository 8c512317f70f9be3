"""CPU tests of the tolerant match's restatement (tests/tol_ref.py): its two forms agree, at tol 0 it gives the
reference's recorded answers, and the numbers that motivate the tolerance follow from showinfo's %.6g rule."""
import json
import math
import os

import numpy as np
import pytest

from tests import tol_ref

ROOT = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(ROOT, "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _rows(corpus):
    return [(int(v), [float("nan") if x is None else float(x) for x in t]) for v, t in corpus]


def _both(rows, q, tol, mm, excl=-1):
    a = tol_ref.find_duplicates_tol(rows, q, tol, mm, excl, form="brute")
    b = tol_ref.find_duplicates_tol(rows, q, tol, mm, excl, form="sorted")
    assert a == b, (a, b)
    return a


@pytest.mark.parametrize("mm", [-1, 0, 1, 2, 5, 6, 40])
def test_forms_agree_on_edge_cases(mm):
    for name, rows, q, tol in tol_ref.edge_rows_and_queries():
        for excl in (-1, 1):
            _both(rows, q, tol, mm, excl)


def test_edge_case_answers_by_hand():
    t = 0.001
    inf, nan = float("inf"), float("nan")
    assert _both([(1, [1.0, 2.0])], [nan, 1.0, nan, 2.0005], t, 1) == [(1, 2, 1)]
    assert _both([(1, [inf, -inf]), (2, [1e308])], [inf, -inf, 1.7976931348623157e308], t, 1) == [(1, 2, 0)]
    assert _both([(1, [10.0])], [10.0 + t, np.nextafter(10.0 + t, 20.0)], t, 1) == [(1, 1, 0)]
    assert _both([(1, [5.0, 5.0004, 5.0008])], [5.0004], t, 1) == [(1, 1, 0)]          # counted once
    assert _both([(1, [5.0])], [4.9995, 5.0005], t, 2) == [(1, 2, 1)]                   # one key, two windows
    assert _both([(1, [1.0, 7.0])], [1.0, 1.0, 1.0005, 7.0], t, 5) == []
    assert _both([(1, [1.0, 7.0])], [1.0, 1.0, 1.0005, 7.0], t, 4) == [(1, 4, 3)]
    assert _both([(1, []), (2, [1.0])], [], t, 0) == [(1, 0, -1), (2, 0, -1)]
    assert _both([(1, [-1.0, -0.0004]), (2, [0.0009])], [0.0, -1.0005], t, 2) == [(1, 2, 1)]


@pytest.mark.parametrize("seed", range(6))
def test_forms_agree_on_random_corpora(seed):
    rng = np.random.default_rng(seed)
    fps = [24, 25, 30][seed % 3]
    grid = np.arange(-300, 3000) / fps
    rows = []
    for v in range(40):
        n = int(rng.integers(0, 60))
        ts = rng.choice(grid, size=n, replace=False) + rng.normal(0, 0.002, size=n) * (v % 2)
        rows.append((v, ts.tolist()))
    for _ in range(8):
        q = rng.choice(grid, size=int(rng.integers(0, 80))) + rng.normal(0, 0.001, size=1)
        for tol in (0.0, 1e-4, 0.001, 0.02, 0.1):
            for mm in (0, 1, 2, 3, 6):
                _both(rows, q.tolist(), tol, mm, excl=int(rng.integers(-1, 40)))


def test_tol_zero_reproduces_the_golden_fixtures():
    """tol 0 is the exact verdict: the reference's recorded (video_id, count) answers, both forms."""
    g = _load("match_kat.json")
    for case in g["cases"] + [g["nan_case"]]:
        q = [float("nan") if x is None else x for x in case["query"]]
        got = _both(_rows(case["corpus"]), q, 0.0, case["min_match"])
        assert [(v, c) for v, c, _ in got] == [tuple(e) for e in case["expected"]], case["name"]
    g = _load("match_random.json")
    for case in g["cases"]:
        rows = _rows(g["corpora"][str(case["corpus_ref"])])
        got = _both(rows, case["query"], 0.0, case["min_match"])
        assert [(v, c) for v, c, _ in got] == [tuple(e) for e in case["expected"]], case["name"]
    g = _load("match_streaming.json")
    for case in g["cases"]:
        dedup = []
        for ts in case["stream"]:
            if not dedup or ts != dedup[-1]:
                dedup.append(ts)
        hits = _both(_rows(case["corpus"]), dedup, 0.0, case["min_match"], case["self_id"])
        if not hits:
            assert case["dup_ids"] == [] and case["scene_timestamps"] == dedup
            continue
        kstar = min(k for _, _, k in hits)
        assert sorted(v for v, _, k in hits if k == kstar) == case["dup_ids"], case["name"]
        assert dedup[:kstar + 1] == case["scene_timestamps"], case["name"]


def test_remux_numbers_from_the_printed_pts_time():
    """30 fps muxed with time base 1/15360 (mp4) and 1/1000 (mkv): in the first 100 s only 999 of 2,999 frames
    print the same pts_time, frame 301 prints 10.0333 against 10.033, and no difference exceeds 0.34 ms."""
    mp4 = [tol_ref.pts_time(512 * i, 1, 15360) for i in range(1, 3000)]
    mkv = [tol_ref.pts_time(round(i * 1000 / 30), 1, 1000) for i in range(1, 3000)]
    assert sum(a == b for a, b in zip(mp4, mkv)) == 999
    assert (mp4[300], mkv[300]) == (10.0333, 10.033)
    worst = max(abs(a - b) for a, b in zip(mp4, mkv))
    assert 0.00033 < worst <= 0.00034
    # so the exact verdict misses two thirds of the cuts, a 1 ms tolerance none of them
    rows = [(1, mp4)]
    assert tol_ref.find_duplicates_tol(rows, mkv, 0.0, 1, form="sorted")[0][1] == 999
    assert tol_ref.find_duplicates_tol(rows, mkv, 0.001, 1, form="sorted")[0][1] == 2999


def test_frame_rate_conversion_numbers_from_the_printed_pts_time():
    """30 -> 25 fps, a cut landing on the first 25 fps frame at or after it: the printed values agree only where the
    two frame grids meet (one cut time in six; 148 of 1,000 random cut times in the issue's draw, 160-185 in these
    seeded draws), and the worst gap is one 30 fps frame, 33.3 ms."""
    def pair(t):
        return tol_ref.pts_time(math.ceil(t * 30), 1, 30), tol_ref.pts_time(math.ceil(t * 25), 1, 25)
    # a cut on 30 fps frame i lands on 25 fps frame ceil(5 i / 6): the same instant exactly when 6 divides i
    grid = [(tol_ref.pts_time(i, 1, 30), tol_ref.pts_time(-(-5 * i // 6), 1, 25)) for i in range(1, 3001)]
    assert sum(a == b for a, b in grid) == 500
    for seed in range(3):
        ts = np.random.default_rng(seed).uniform(0, 600, 1000)
        pr = [pair(float(t)) for t in ts]
        same = sum(a == b for a, b in pr)
        assert 120 <= same <= 200, same
        worst = max(abs(a - b) for a, b in pr)
        assert 0.0332 < worst <= 0.03334
