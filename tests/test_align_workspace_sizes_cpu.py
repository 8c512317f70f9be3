"""The alignment top-k's other five sizing functions, pure arithmetic (no GPU), against recorded answers - the sibling
of tests/test_workspace_sizes_cpu.py, which holds tvz_align_topk_workspace_bytes: the sharded form of the bounded call,
the wide call and its sharded form, the call with rates and the call with spans.  Every byte count is part of the ABI.
tests/golden/align_workspace_sizes.json holds the spelled-out shapes (a failure names one) and a SHA-256 over the
answers of the whole grid below.

The grid is the sibling's (its Q, max_query_len, k and key counts; these functions take no cap), with n_ranks in
(-1, 0, 1, 8): tvz_align_topk_sharded_workspace_bytes answers 0 to a negative n_ranks, and
tvz_align_wide_topk_sharded_workspace_bytes sizes it as one rank.  Callers may rely on either, so both are held here.

The fixture was recorded from the library as it was before its host code learned of a form from one table.  Record it
again (python -m tests.test_align_workspace_sizes_cpu --record) only from a library whose sizes are meant to be the new
ABI."""
import hashlib
import itertools
import json
import os
import sys

import pytest

from tests import test_workspace_sizes_cpu as base
from tvidz_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_workspace_sizes.json")

QS, LENS, KS, N_KEYS = base.QS, base.LENS, base.KS, base.N_KEYS
RANKS = (-1, 0, 1, 8)

# name -> the arguments it takes, in its own order
FUNCTIONS = (
    ("tvz_align_topk_sharded_workspace_bytes", ("Q", "L", "keys", "k", "n_ranks")),
    ("tvz_align_wide_topk_workspace_bytes", ("Q", "L", "keys", "k")),
    ("tvz_align_wide_topk_sharded_workspace_bytes", ("Q", "L", "keys", "k", "n_ranks")),
    ("tvz_align_rates_topk_workspace_bytes", ("Q", "L", "keys", "k")),
    ("tvz_align_span_topk_workspace_bytes", ("Q", "L", "keys", "k")),
)

# the spelled-out shapes: (Q, L, k, n_ranks, keys); every function is asked about each
NAMED = (
    (0, 0, 0, 0, 0), (1, 5, 16, 1, 5), (2, 260, 16, 8, 527), (1024, 260, 64, 8, 0), (1024, 260, 65, 8, 0),
    (65535, 5, 1024, 1, 0), (65, 4096, 16, 1, 4096), (3, 10000, 4, 1, 30007), (-1, 260, 16, 1, 0), (2, 260, 16, -1, 527),
    (64, 4095, 64, 0, 0),
)


def _shapes():
    for Q, L, k, n_ranks, which in itertools.product(QS, LENS, KS, RANKS, range(N_KEYS)):
        yield Q, L, k, n_ranks, (0, L, Q * L + 7)[which]


def _ask(lib, name, names, shape):
    by_name = dict(zip(("Q", "L", "k", "n_ranks", "keys"), shape))
    return int(getattr(lib, name)(*[by_name[a] for a in names]))


def _grid_digest(lib):
    h = hashlib.sha256()
    for shape in _shapes():
        for name, names in FUNCTIONS:
            h.update(b"%d\n" % _ask(lib, name, names, shape))
    return h.hexdigest()


def _named(lib):
    return [{"function": name, "Q": s[0], "max_query_len": s[1], "k": s[2], "n_ranks": s[3], "total_query_keys": s[4],
             "bytes": _ask(lib, name, names, s)} for s in NAMED for name, names in FUNCTIONS]


def _grid():
    return {"Q": list(QS), "max_query_len": list(LENS), "k": list(KS), "n_ranks": list(RANKS),
            "total_query_keys": ["0", "max_query_len", "Q * max_query_len + 7"], "functions": [n for n, _ in FUNCTIONS]}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_spelled_out_shapes(recorded):
    got = _named(_lib.load())
    assert len(recorded["named"]) == len(NAMED) * len(FUNCTIONS)
    assert [dict(e, bytes=None) for e in got] == [dict(e, bytes=None) for e in recorded["named"]]   # the same questions
    for g, e in zip(got, recorded["named"]):
        assert g["bytes"] == e["bytes"], (g, e["bytes"])


def test_a_negative_rank_count(recorded):
    """The two sharded sizing functions differ on n_ranks < 0, and the fixture says how: the bounded one refuses it
    (0), the wide one sizes it as one rank."""
    by = {(e["function"], e["n_ranks"]): e["bytes"] for e in recorded["named"]
          if (e["Q"], e["max_query_len"], e["k"], e["total_query_keys"]) == (2, 260, 16, 527)}
    assert by["tvz_align_topk_sharded_workspace_bytes", -1] == 0
    lib = _lib.load()
    assert by["tvz_align_wide_topk_sharded_workspace_bytes", -1] \
        == int(lib.tvz_align_wide_topk_sharded_workspace_bytes(2, 260, 527, 16, 1)) > 0


def test_the_whole_grid(recorded):
    assert recorded["grid"] == _grid()
    assert _grid_digest(_lib.load()) == recorded["sha256"]


if __name__ == "__main__" and "--record" in sys.argv:
    lib = _lib.load()
    doc = {"grid": _grid(),
           "order": "itertools.product over the grid's lists in the order above, per shape the functions in their order, "
                    "each answer as decimal digits and a newline",
           "sha256": _grid_digest(lib), "named": _named(lib)}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(FIXTURE, len(doc["named"]), doc["sha256"])
