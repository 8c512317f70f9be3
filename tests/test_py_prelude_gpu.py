"""The one prelude of corpus.py's batched wrappers, asked through each of the thirteen that need no communicator (the
three of corpus.Comm are asked in tests/test_comm_gpu.py's child process): tests/prelude_cases.py says what."""
import pytest

from tests import prelude_cases as pc
from tvidz_amd import corpus as tc

pytestmark = pytest.mark.gpu
NAMES = ["match", "match_tol", "match_topk", "match_tol_topk", "align_topk_block", "match_topk_shards",
         "align_topk_shards", "align_wide_topk_block", "align_rates_topk_block", "align_span_topk_block",
         "align_wide_topk_shards", "align_rates_topk_shards", "align_span_topk_shards"]


@pytest.fixture(scope="module")
def shards():
    handles = [tc.DeviceCorpus(0), tc.DeviceCorpus(0)]
    handles[0].upload(pc.ROWS[:3])
    handles[1].upload(pc.ROWS[3:])
    yield handles
    for h in handles:
        h.close()


@pytest.mark.parametrize("name", NAMES)
def test_wrapper_refuses_before_the_library_and_takes_an_exact_workspace(shards, name):
    specs = pc.wrappers(shards)
    assert sorted(specs) == sorted(NAMES)
    assert pc.failures(name, *specs[name]) == []
