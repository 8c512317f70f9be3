"""The batched calls keep inside the workspace they are given.  Every call that carves a workspace - tvz_match,
tvz_match_topk, tvz_match_tol, tvz_match_tol_topk, tvz_align_topk and its wide, rates and span forms - gets a slice of
EXACTLY its sizing function's byte count out of a larger buffer filled with 0xA5, starting 4,096 bytes in plus 0, 8 or 248 bytes (the carver aligns the
base up itself); afterwards every byte outside the slice is still 0xA5, and the outputs equal those of the same call
with a separately allocated workspace of twice the size.

This test is about pointers: it compares the library with itself, on purpose (the answers are held by the other
suites).  Top-k blocks are ordered and compared as they are.  The order inside a hit list is unspecified (blocks append
with atomics), so the lists of tvz_match and tvz_match_tol are compared as counts plus sorted triples; every query here
has fewer hits than `cap`, so both runs hold the whole list."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP, K, LEAD = 64, 4, 4096
CELL, TOL = 0.001, 0.0005
EXTRA = (0, 8, 248)
GRID = 3000                                                 # timestamps are multiples of 0.25 s below 750 s


def _rows():
    rng = np.random.RandomState(11)
    return [(100 + r, (np.sort(rng.choice(GRID, size=rng.randint(1, 13), replace=False)) * 0.25).tolist())
            for r in range(320)]


def _corpus(kind):
    """plain: 300 rows upserted one by one (too few for an index).  delta: 300 rows uploaded (which builds the
    index), 20 more upserted afterwards.  cells: the same with cell postings (tvz_corpus_tol_index) on."""
    rows = _rows()
    dc = tc.DeviceCorpus(0)
    if kind == "plain":
        for vid, ts in rows[:300]:
            dc.upsert(vid, ts)
        assert dc.index_stats()["indexed_rows"] == 0
        return dc
    if kind == "cells":
        dc.set_tol_index(CELL)
    dc.upload(rows[:300])
    for vid, ts in rows[300:]:
        dc.upsert(vid, ts)
    st = dc.index_stats()
    assert st["indexed_rows"] == 300 and st["delta_rows"] == 20
    assert (dc.tol_index_stats()["postings"] > 0) == (kind == "cells")
    return dc


@functools.lru_cache(maxsize=None)
def _batch(long):
    rows = _rows()
    if long:      # one query of 4,100 timestamps: off the corpus' grid but for two rows' worth (one of them in the delta)
        q = [x * 0.25 + 0.1 for x in range(4100 - len(rows[7][1]) - len(rows[310][1]))] + rows[7][1] + rows[310][1]
        qs = [q]
    else:         # Q = 3, one of them empty; the others hold an indexed row's and a delta row's timestamps
        qs = [(rows[5][1] + rows[40][1])[:12], [], (rows[305][1] + rows[200][1])[:12]]
    d_q, d_off, longest = tc.pack_queries(qs, DEV)
    return d_q, d_off, (4100 if long else 12), len(qs)


def _lists(hits, n):
    torch.cuda.synchronize()
    hits, n = hits.cpu().numpy(), n.cpu().numpy()
    assert n.max() < CAP and n.max() > 0, n
    return [(int(n[q]), sorted(map(tuple, hits[q, :int(n[q])].tolist()))) for q in range(len(n))]


def _block(out):
    torch.cuda.synchronize()
    return out.cpu().numpy().tolist()


# call -> (bytes the sizing function asks for, the call with that workspace -> comparable outputs)
def _match(dc, b, ws):
    return _lists(*dc.match(b[0], b[1], b[2], 1, CAP, workspace=ws))


def _match_topk(dc, b, ws):
    return _block(dc.match_topk(b[0], b[1], b[2], 1, CAP, K, workspace=ws))


def _match_tol(dc, b, ws):
    return _lists(*dc.match_tol(b[0], b[1], b[2], TOL, 1, CAP, workspace=ws))


def _match_tol_topk(dc, b, ws):
    return _block(dc.match_tol_topk(b[0], b[1], b[2], TOL, 1, K, workspace=ws))


def _align_topk(dc, b, ws):
    out = torch.empty((b[3], K + 1, 4), dtype=torch.int32, device=DEV)
    _lib.check(dc.lib.tvz_align_topk(dc._h, b[0].data_ptr(), b[1].data_ptr(), b[3], b[2], 0.05, 1.0, 1, 0, None, K,
                                     out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    return _block(out)


RATES = (1.0, 25 / 24)


def _align_wide_topk(dc, b, ws):
    out = torch.empty((b[3], K + 1, 4), dtype=torch.int32, device=DEV)
    _lib.check(dc.lib.tvz_align_wide_topk(dc._h, b[0].data_ptr(), b[1].data_ptr(), b[3], b[2], 0.05, 1.0, 1, 0, 0, None, K,
                                          out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream().cuda_stream))
    return _block(out)


def _align_rates_topk(dc, b, ws):
    out = torch.empty((b[3], K + 1, 5), dtype=torch.int32, device=DEV)
    _lib.check(dc.lib.tvz_align_rates_topk(dc._h, b[0].data_ptr(), b[1].data_ptr(), b[3], b[2], 0.05, 1.0,
                                           (C.c_double * len(RATES))(*RATES), len(RATES), 1, 0, 0, None, K, out.data_ptr(),
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    return _block(out)


def _align_span_topk(dc, b, ws):
    out = torch.empty((b[3], K + 1, 8), dtype=torch.int32, device=DEV)
    _lib.check(dc.lib.tvz_align_span_topk(dc._h, b[0].data_ptr(), b[1].data_ptr(), b[3], b[2], 0.05, 1.0,
                                          (C.c_double * len(RATES))(*RATES), len(RATES), 1, 0, 0, None, K, out.data_ptr(),
                                          ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    return _block(out)


CALLS = {
    "match": (lambda b: tc.workspace_bytes(b[3], b[2], 0, 0, 1, b[0].numel()), _match),
    "match_topk": (lambda b: tc.workspace_bytes(b[3], b[2], CAP, K, 1, b[0].numel()), _match_topk),
    "match_tol": (lambda b: tc.tol_workspace_bytes(b[3], b[2], b[0].numel()), _match_tol),
    "match_tol_topk": (lambda b: tc.tol_topk_workspace_bytes(b[3], b[2], b[0].numel(), K, 1), _match_tol_topk),
    "align_topk": (lambda b: tc.align_topk_workspace_bytes(b[3], b[2], b[0].numel(), K), _align_topk),
    "align_wide_topk": (lambda b: tc.align_wide_topk_workspace_bytes(b[3], b[2], b[0].numel(), K), _align_wide_topk),
    "align_rates_topk": (lambda b: tc.align_rates_topk_workspace_bytes(b[3], b[2], b[0].numel(), K), _align_rates_topk),
    "align_span_topk": (lambda b: tc.align_span_topk_workspace_bytes(b[3], b[2], b[0].numel(), K), _align_span_topk),
}


class World:
    """the three handles, and per (call, handle, batch) the answer with a workspace of its own, twice the size: each
    made once, at its first use"""

    def __init__(self):
        self.handles, self.answers = {}, {}

    def corpus(self, kind):
        if kind not in self.handles:
            self.handles[kind] = _corpus(kind)
        return self.handles[kind]

    def reference(self, call, kind, long):
        if (call, kind, long) not in self.answers:
            need, run = CALLS[call]
            b = _batch(long)
            ws = torch.empty(2 * need(b), dtype=torch.uint8, device=DEV)
            self.answers[call, kind, long] = run(self.corpus(kind), b, ws)
        return self.answers[call, kind, long]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    for dc in w.handles.values():
        dc.close()


CASES = [(call, kind, False) for call in CALLS for kind in ("plain", "delta")] + \
        [(call, "cells", False) for call in ("match_tol", "match_tol_topk")] + \
        [(call, kind, True) for call in ("match", "match_topk") for kind in ("plain", "delta")]


@pytest.mark.parametrize("extra", EXTRA)
@pytest.mark.parametrize("call,kind,long", CASES)
def test_the_call_stays_inside_its_slice(world, call, kind, long, extra):
    need, run = CALLS[call]
    b = _batch(long)
    n = need(b)
    assert n > 0
    buf = torch.full((LEAD + 256 + n + LEAD,), 0xA5, dtype=torch.uint8, device=DEV)
    lo, hi = LEAD + extra, LEAD + extra + n
    got = run(world.corpus(kind), b, buf[lo:hi])
    torch.cuda.synchronize()
    assert bool((buf[:lo] == 0xA5).all()), f"{call}: bytes in front of the workspace were written"
    assert bool((buf[hi:] == 0xA5).all()), f"{call}: bytes behind the workspace were written"
    assert got == world.reference(call, kind, long)
