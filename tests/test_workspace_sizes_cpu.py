"""The five workspace sizing functions, pure arithmetic (no GPU), against recorded answers: callers size buffers with
them, so every byte count - alignment slack included - is part of the ABI.  tests/golden/workspace_sizes.json holds
about forty spelled-out shapes (a failure names one) and a SHA-256 over the answers of the whole grid below.

The fixture was recorded from the library as it was before the layouts moved onto one carver.  Record it again
(python -m tests.test_workspace_sizes_cpu --record) only from a library whose sizes are meant to be the new ABI.

(That a workspace of tvz_match_tol_workspace_bytes(Q, L, keys) bytes is accepted for exactly `keys` values cannot be
asked here: every call that takes a workspace needs a handle, and a handle needs a device.
tests/test_workspace_bounds_gpu.py passes exactly-sized workspaces.)"""
import hashlib
import itertools
import json
import os
import sys

import pytest

from tvidz_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")

QS = (0, 1, 2, 63, 64, 65, 1024, 65535, -1)
LENS = (0, 1, 5, 260, 4095, 4096, 10000)
CAPS = (0, 1, 4096)
KS = (0, 1, 16, 64, 65, 1024)
RANKS = (0, 1, 8)
N_KEYS = 3                                 # total_query_keys: 0, max_query_len, Q * max_query_len + 7

# name -> the arguments it takes, in its own order
FUNCTIONS = (
    ("tvz_match_workspace_bytes", ("Q", "L", "cap", "k", "n_ranks")),
    ("tvz_match_workspace_bytes_long", ("Q", "L", "cap", "k", "n_ranks", "keys")),
    ("tvz_match_tol_workspace_bytes", ("Q", "L", "keys")),
    ("tvz_match_tol_topk_workspace_bytes", ("Q", "L", "keys", "k", "n_ranks")),
    ("tvz_align_topk_workspace_bytes", ("Q", "L", "keys", "k")),
)

# the spelled-out shapes: (Q, L, cap, k, n_ranks, keys); every function is asked about each
NAMED = (
    (0, 0, 0, 0, 0, 0), (1, 5, 4096, 16, 1, 5), (2, 260, 4096, 16, 8, 527), (1024, 260, 4096, 64, 8, 0),
    (1024, 260, 4096, 65, 8, 0), (65535, 5, 1, 1024, 1, 0), (65, 4096, 4096, 16, 1, 4096), (3, 10000, 64, 4, 1, 30007),
    (1, 10000, 0, 0, 0, 10000), (-1, 260, 4096, 16, 1, 0),
)


def _shapes():
    for Q, L, cap, k, n_ranks, which in itertools.product(QS, LENS, CAPS, KS, RANKS, range(N_KEYS)):
        yield Q, L, cap, k, n_ranks, (0, L, Q * L + 7)[which]


def _ask(lib, name, names, shape):
    by_name = dict(zip(("Q", "L", "cap", "k", "n_ranks", "keys"), shape))
    return int(getattr(lib, name)(*[by_name[a] for a in names]))


def _grid_digest(lib):
    h = hashlib.sha256()
    for shape in _shapes():
        for name, names in FUNCTIONS:
            h.update(b"%d\n" % _ask(lib, name, names, shape))
    return h.hexdigest()


def _named(lib):
    return [{"function": name, "Q": s[0], "max_query_len": s[1], "cap": s[2], "k": s[3], "n_ranks": s[4],
             "total_query_keys": s[5], "bytes": _ask(lib, name, names, s)}
            for s in NAMED for name, names in FUNCTIONS if name != "tvz_match_workspace_bytes_long" or s[1] > 4095]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_spelled_out_shapes(recorded):
    got = _named(_lib.load())
    assert len(recorded["named"]) >= 40
    assert [dict(e, bytes=None) for e in got] == [dict(e, bytes=None) for e in recorded["named"]]   # the same questions
    for g, e in zip(got, recorded["named"]):
        assert g["bytes"] == e["bytes"], (g, e["bytes"])


def test_the_whole_grid(recorded):
    assert recorded["grid"] == {"Q": list(QS), "max_query_len": list(LENS), "cap": list(CAPS), "k": list(KS),
                                "n_ranks": list(RANKS), "total_query_keys": ["0", "max_query_len", "Q * max_query_len + 7"],
                                "functions": [n for n, _ in FUNCTIONS]}
    assert _grid_digest(_lib.load()) == recorded["sha256"]


if __name__ == "__main__" and "--record" in sys.argv:
    lib = _lib.load()
    doc = {"grid": {"Q": list(QS), "max_query_len": list(LENS), "cap": list(CAPS), "k": list(KS), "n_ranks": list(RANKS),
                    "total_query_keys": ["0", "max_query_len", "Q * max_query_len + 7"],
                    "functions": [n for n, _ in FUNCTIONS]},
           "order": "itertools.product over the grid's lists in the order above, per shape the functions in their order, "
                    "each answer as decimal digits and a newline",
           "sha256": _grid_digest(lib), "named": _named(lib)}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(FIXTURE, len(doc["named"]), doc["sha256"])
