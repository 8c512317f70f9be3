"""tvz_match_tol_topk_workspace_bytes, pure arithmetic (no GPU): the workspace of the form that keeps the top-k in
the sweep is no larger than what the path it replaces needs at the service's default cap of 4,096 hits per query;
it grows with every argument; nonsense arguments answer 0 as the sibling functions do."""
import itertools

import pytest

from tvidz_amd import _lib, corpus as tc

CAP = 4096                                 # service.py's default --cap
SLACK = 8 * 256                            # alignment: a handful of 256-byte roundings on either side


def test_the_entry_points_are_bound():
    lib = _lib.load()
    assert _lib.VERSION == 404 and lib.tvz_version() == 404
    for name in ("tvz_match_tol_topk_workspace_bytes", "tvz_match_tol_topk", "tvz_match_tol_sharded"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("Q,k,n_ranks", itertools.product((64, 256, 1024, 4096), (1, 16, 64), (1, 8)))
def test_no_larger_than_the_hit_list_path_it_replaces(Q, k, n_ranks):
    for L, keys in ((200, 0), (200, Q * 37), (4095, 0), (1, 0)):
        new = tc.tol_topk_workspace_bytes(Q, L, keys, k, n_ranks)
        old = tc.tol_workspace_bytes(Q, L, keys) + Q * CAP * 12 + (n_ranks + 1) * Q * (k + 1) * 12
        assert 0 < new <= old + SLACK, (Q, k, n_ranks, L, keys, new, old)
        # what it is made of: the sorted queries, at most 96 (the rule gives 95) kept lists per query, the blocks
        assert new >= tc.tol_workspace_bytes(Q, L, keys) + (n_ranks + 1) * Q * (k + 1) * 12
        assert new <= tc.tol_workspace_bytes(Q, L, keys) + Q * 96 * k * 8 + 4 * Q + (n_ranks + 1) * Q * (k + 1) * 12 + SLACK


def test_monotone_in_every_argument():
    base = dict(Q=64, max_query_len=200, total_query_keys=0, k=16, n_ranks=2)
    steps = dict(Q=(1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1000, 1024, 4096, 65535), max_query_len=(0, 1, 200, 4095),
                 total_query_keys=(1, 100, 12800, 10**6), k=(1, 2, 16, 63, 64), n_ranks=(1, 2, 8, 64))
    for name, values in steps.items():
        sizes = [tc.tol_topk_workspace_bytes(**dict(base, **{name: v})) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (name, sizes)
    # n_ranks 0 and 1 both mean one gathered block
    assert tc.tol_topk_workspace_bytes(64, 200, 0, 16, 0) == tc.tol_topk_workspace_bytes(64, 200, 0, 16, 1)


def test_nonsense_arguments_answer_zero():
    f = tc.tol_topk_workspace_bytes
    assert f(-1, 200, 0, 16, 1) == 0 and f(64, -1, 0, 16, 1) == 0 and f(64, 200, -1, 16, 1) == 0
    assert f(64, 200, 0, 0, 1) == 0 and f(64, 200, 0, -3, 1) == 0 and f(64, 200, 0, 16, -1) == 0
    assert tc.tol_workspace_bytes(-1, 200, 0) == 0                         # the sibling's answer
