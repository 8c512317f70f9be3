"""The near-duplicate search with rates, with spans and the parts call through RCCL at world size 1, and the Inspector
over a one-rank service.RankCorpus(RcclShardedMatcher), in ONE fresh child process that creates the communicator before
its first GPU call (tests/near_service_comm_child.py).  Every comparison is of exact integers: a sharded call equals its
unsharded call bit for bit; a gather of the wrong width would show as a half-filled block.  No machine here has two GPUs:
the calls are unrun at more than one rank (their merges are tested with up to 16 hand-made lists, the collective order
over gloo)."""
import json
import os
import subprocess
import sys

import pytest

from tests import align_parts_cases as cs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h
SIZERS = {"align_rates_topk": "tvz_align_rates_topk_sharded_workspace_bytes", "align_span_topk": "tvz_align_span_topk_sharded_workspace_bytes",
          "align_parts": "tvz_align_parts_sharded_workspace_bytes"}


@pytest.fixture(scope="module")
def comm_child():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "near_service_comm_child.py")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_the_three_sharded_calls_equal_their_unsharded_calls(comm_child):
    res = comm_child
    assert len(res["equal"]) == 3 * 2 * (1 + 4 + 2) + 1
    assert all(res["equal"].values()), [n for n, ok in res["equal"].items() if not ok]
    # the premises: the searches hit (more often than k = 5 for the plain one), the over-long query is refused, the excluded
    # id is gone, and the named ids hold parts, a refusal and an absent id
    plain, local, excluded = (res["premise"][n] for n in ("plain", "local", "local excluded"))
    assert max(plain["totals"][:5]) > 5 and plain["totals"][5] == INT32_MIN
    assert local["first_ids"][0] == cs.FILM and excluded["first_ids"][0] != cs.FILM
    assert excluded["totals"][0] == local["totals"][0] - 1 and excluded["totals"][1:] == local["totals"][1:]
    n_parts, n_rows = res["premise"]["parts"]["n_parts"], res["premise"]["parts"]["n_rows"]
    film, nine, absent = cs.IDS.index(cs.FILM), cs.IDS.index(cs.NINE_ROWS), cs.IDS.index(cs.ABSENT)
    assert n_parts[0][film] == 2 and n_parts[2][film] == 2                         # the insertion, at either speed
    assert n_parts[0][nine] == INT32_MIN and n_rows[0][nine] == 9 and n_rows[0][absent] == 0
    assert all(v == INT32_MIN for v in n_parts[5][:absent + 1])                   # the over-long query: every pair refused


def test_the_matcher_answers_all_four_forms_and_parts_on_every_side_stream(comm_child):
    res = comm_child
    assert res["matcher_forms"] == ["align_topk", "align_wide_topk", "align_rates_topk", "align_span_topk"]
    assert res["matcher_supports"] == [True, True, True]
    assert res["matcher_slots_equal"] == [True, True, True]


@pytest.mark.parametrize("stem", sorted(SIZERS))
def test_workspace_bounds_and_the_refusals_behind_the_unsharded_calls(comm_child, stem):
    b = comm_child["bounds"][stem]
    sharded_size, least, plain_size = b["sizes"]
    assert b["exact"] == [True, True, True] and least <= sharded_size and sharded_size > plain_size
    rc, msg = b["short"]
    assert rc == ERR_WORKSPACE and " 1 bytes missing" in msg and SIZERS[stem] in msg, msg
    assert b["least_ok"] == 0
    rc, msg = b["null_comm"]
    assert rc == ERR_INVALID and "communicator is NULL" in msg, msg
    # the unsharded call's refusals come first, in its words: the rate list, then the workspace; the communicator's behind
    rc, msg = b["null_comm_and_no_rates"]
    assert rc == ERR_UNSUPPORTED and "n_rates=0 outside 1..8" in msg, msg
    rc, msg = b["null_comm_and_short"]
    assert rc == ERR_WORKSPACE and SIZERS[stem] in msg, msg
    if stem == "align_parts":
        rc, msg = b["parts5"]
        assert rc == ERR_UNSUPPORTED and "max_parts=5 outside 1..4" in msg, msg
    else:
        rc, msg = b["bad_flag"]
        assert rc == ERR_INVALID and "unknown flag bits 0x4" in msg, msg
        rc, msg = b["k65"]
        assert rc == ERR_UNSUPPORTED and "k=65 outside 1..64" in msg, msg
    assert b["nothing_written"] is True


def test_inspector_over_a_one_rank_rank_corpus(comm_child):
    res = comm_child
    assert res["rank_supports"] == [True, True, True, True] and res["rank_broken"] is None
    assert res["near_rank"] == res["near_plain"]
    near = res["near_rank"]
    # the 24 -> 25 fps copy: reported with its rate, invisible at one speed
    (fps,) = near["fps"]
    assert fps["video_id"] == cs.FILM and fps["rate"] == 25.0 / 24.0 and fps["jaccard"] == 1.0
    assert abs(fps["shift_seconds"] + 12.3 * 25.0 / 24.0) <= cs.EPS and near["fps_unrated"] == []
    # the 20-cut clip inside a 400-cut compilation: only the local score finds it
    assert near["compilation_containment"] == []
    (clip,) = near["compilation_local"]
    assert clip["video_id"] == 500 and clip["local"] == 1.0 and clip["jaccard"] == round(20 / 780, 4)
    # the upload with an inserted segment: both halves, under near_parts=2
    (ins,) = near["inserted_parts"]
    assert ins["video_id"] == cs.FILM and ins["parts_score"] == 1.0 and [p["votes"] for p in ins["parts"]] == [60, 60]
    assert [p["shift_seconds"] for p in ins["parts"]] == [0.0, -1419 * cs.EPS]


def test_the_caller_refuses_and_answers_over_long_queries_without_a_tick(comm_child):
    c = comm_child["caller"]
    assert c["refused"] == ["ValueError"] * 5 and c["ticks_unchanged"] is True
    assert c["long_totals"] == [INT32_MIN]
    assert c["long_parts"] == [[[[cs.FILM, 0, 0, INT32_MIN, 0, 0], [0] * 6, [0] * 6], [[-1, 0, 0, 0, 0, 0], [0] * 6, [0] * 6]]]
