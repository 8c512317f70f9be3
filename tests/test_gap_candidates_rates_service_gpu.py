"""The rates candidates call through RCCL at world size 1, and the Inspector with near_candidate_rates over a one-rank
service.RankCorpus(RcclShardedMatcher), in ONE fresh child process - a subprocess under its own timeout - that creates the
communicator before its first GPU call (tests/gap_candidates_rates_comm_child.py).  Every comparison is of exact
integers: the sharded call equals the plain rates call bit for bit; a gather of the wrong width would show as a
part-filled block.  No machine here has two GPUs: the call is never run on more than one GPU (its merge is tested with
up to 16 hand-made lists)."""
import json
import os
import subprocess
import sys

import pytest

from tests import gap_candidates_rates_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MIN = -(1 << 31)
ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -4, -5           # include/tvz.h


@pytest.fixture(scope="module")
def comm_child():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gap_candidates_rates_comm_child.py")], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_the_sharded_call_equals_the_plain_rates_call(comm_child):
    res = comm_child
    assert len(res["equal"]) == 3 * 3 * 3 + 1
    assert all(res["equal"].values()), [n for n, ok in res["equal"].items() if not ok]
    at = {n: i for i, n in enumerate(rc.NAMES)}
    assert res["first"][at["slow"]] == [rc.FILM, 117, 1] and res["first"][at["fast"]] == [rc.FILM, 117, 2]


def test_the_matcher_answers_on_every_side_stream(comm_child):
    assert comm_child["matcher_supports"] is True and comm_child["matcher_slots_equal"] == [True, True, True]


def test_the_workspace_bounds_and_the_refusals_behind_the_plain_calls(comm_child):
    b = comm_child["bounds"]
    n, least, plain = b["sizes"]
    assert b["exact"] == [True, True, True] and least <= n and plain < n
    rc_, msg = b["short"]
    assert rc_ == ERR_WORKSPACE and " 1 bytes missing (size it with tvz_align_candidates_rates_sharded_workspace_bytes)" in msg
    # the NULL communicator stands behind every refusal of the plain call
    assert b["null_comm"][0] == ERR_INVALID and "communicator is NULL" in b["null_comm"][1]
    assert b["null_comm_and_c65"][0] == ERR_UNSUPPORTED and "C=65" in b["null_comm_and_c65"][1]
    assert b["null_comm_and_rates"][0] == ERR_UNSUPPORTED and "n_rates=9" in b["null_comm_and_rates"][1]
    assert b["null_comm_and_short"][0] == ERR_WORKSPACE
    assert b["null_comm_and_no_codes"][0] == ERR_UNSUPPORTED and "keeps no gap codes" in b["null_comm_and_no_codes"][1]
    assert b["null_out"][0] == ERR_INVALID and "d_out is NULL" in b["null_out"][1]
    assert b["nothing_written"] is True


def test_the_inspector_over_a_one_rank_corpus_equals_the_plain_one(comm_child):
    res = comm_child
    assert res["rank_supports"] == [True, True] and res["rank_broken"] is None
    assert res["near_rank"] == res["near_plain"] and len(res["near_plain"]) == 8
    (near,) = res["near_plain"]["slow 0"]
    assert near["video_id"] == rc.FILM and near["rate"] == rc.SLOW
    assert res["near_plain"]["fast 1"][0]["video_id"] == rc.FILM and res["near_plain"]["fast 1"][0]["rate"] == rc.FAST
    assert res["rank_equals_plain"] is True
    c = res["caller"]
    assert c["refused"] == ["ValueError"] * 5 and c["long_totals"] == [INT32_MIN] and c["long_rows_padding"] and c["ticks_unchanged"]
