"""The index lookup kernels at their internal limits (tests/lookup_cases.py: the per-wave posting cache, pass A / pass B
trips, chunks of query positions, parts of candidate slots, the fused top-k's histogram and kept list, the slot modes,
the pair form, the one-wave kernel's register range and probe rounds, sub-index groups) against the oracle's
restatement of db.find_duplicates (oracle.match_kth_csr), bit-exactly: rows ascending by (kth, video_id, count),
padding, totals row.  Every case goes through every form that takes it: ts_match_index_topk_kernel with one and with
two queries per block, ts_match_wq_topk_kernel, ts_match_index_kernel (full hit lists, then tvz_topk_shard of them)
and ts_find_fused_kernel (find_duplicates); the last test asserts that each form ran for every case meant for it.
Not run here: the RCCL forms and anything on more than one GPU."""
import numpy as np
import pytest
import torch

from tests import lookup_cases as cases
from tvidz_amd import _lib, corpus as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEVER = tc.KTH_NEVER
FORMS = ("block", "pair", "wave", "fused", "match", "find", "fixup")
FORM_RUNS = {f: set() for f in FORMS}       # form -> the cases that were compared through it
_EXPECTED = {}                              # (case, phase, min_match, excluded id, query bytes) -> the oracle's hits


def _hits(cs, phase, c, queries, mm, excl):
    """the oracle's hits of every query of a batch, each distinct (query, exclusion) computed once per case"""
    keys = [(cs.name, phase, mm, excl[qi] if excl else None, q.tobytes()) for qi, q in enumerate(queries)]
    todo = {k: qi for qi, k in enumerate(keys) if k not in _EXPECTED}
    new = cases.expected_many(c, [queries[qi] for qi in todo.values()], mm, [k[3] for k in todo])
    _EXPECTED.update(zip(todo, new))
    return [_EXPECTED[k] for k in keys]


def _block(hits, k, cap):
    rows = sorted(hits, key=lambda h: (h[2], h[0], h[1]))[:k]
    rows += [(-1, 0, NEVER)] * (k - len(rows))
    rows.append((-1, len(hits) if len(hits) <= cap else -len(hits), NEVER))
    return np.array(rows, dtype=np.int64).astype(np.int32)


def _same_blocks(got, want, exp, truncated, what):
    """a form's [Q][k + 1][3] answer against the oracle's; a truncated query: the total is negated, the rows are real hits"""
    assert got.shape == want.shape, what
    bad = [qi for qi in np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1)) if qi not in truncated]
    assert not bad, (what, bad[:8], got[bad[0]][:4].tolist(), want[bad[0]][:4].tolist(), got[bad[0]][-1].tolist(),
                     want[bad[0]][-1].tolist())
    for qi in truncated:
        assert tuple(got[qi, -1]) == (-1, -len(exp[qi]), NEVER), (what, qi)
        assert set(tuple(int(x) for x in r) for r in got[qi, :-1] if r[0] >= 0) <= set(exp[qi]), (what, qi)


def _run_batch(dc, cs, phase, c, bi):
    b = cs.batches[bi]
    queries = cases.padded(b)
    Q, real = len(queries), len(b.queries)
    d_q, d_off, longest = tc.pack_queries(queries, DEV)
    max_len = cases.batch_max_len(b)
    assert longest <= max_len
    excl = list(b.excl) + [-1] * (Q - real) if b.excl is not None else None
    d_ex = torch.tensor(excl, dtype=torch.int32, device=DEV) if excl is not None else None
    n_keys = int(d_q.numel())
    for mm, k, cap in b.runs:
        exp = _hits(cs, phase, c, queries, mm, excl)
        assert all(len(e) <= cap for qi, e in enumerate(exp) if qi not in b.truncated)
        want = np.stack([_block(e, k, cap) for e in exp])
        what = (cs.name, phase, bi, mm, k, cap)
        fused = None
        if mm <= cases.CONSTANTS["kTop"] and b.forms is None:
            ws = torch.empty(tc.workspace_bytes(Q, max_len, cap, k, total_query_keys=n_keys), dtype=torch.uint8, device=DEV)
            forms = [("block", _lib.ALGO_NO_WAVE | _lib.ALGO_NO_PAIR), ("pair", _lib.ALGO_PAIR)]
            if cases.wave_usable(cs.corpus.ids.size, cs.n_sub, cs.bucket, max_len, mm, k):
                forms.append(("wave", _lib.ALGO_WAVE))
            for form, algo in forms:
                got = dc.match_topk(d_q, d_off, max_len, mm, cap, k, d_exclude_ids=d_ex, workspace=ws, algo=algo)
                got = got.cpu().numpy()
                _same_blocks(got, want, exp, b.truncated, what + (form,))
                fused = got if form == "block" else fused
                if form == "pair" and not (Q >= 2 and cases.pair_fits(max_len, cs.n_sub)):
                    continue                                     # (the library took the one-query form)
                FORM_RUNS[form].add(cs.name)
            if cases.fused_usable(Q, cs.n_sub, max_len, mm, k):
                FORM_RUNS["fused"].add(cs.name)
        # the unfused lookup: full hit lists and hits_n, then the top-k of them against the fused block
        ws = torch.empty(tc.workspace_bytes(Q, max_len, total_query_keys=n_keys), dtype=torch.uint8, device=DEV)
        hits, n = dc.match(d_q, d_off, max_len, mm, cap, d_exclude_ids=d_ex, workspace=ws, algo=_lib.ALGO_INDEX)
        blk = tc.topk_shard(hits, n, k).cpu().numpy()
        hits, n = hits.cpu().numpy(), n.cpu().numpy()
        for qi in range(Q):
            assert int(n[qi]) == len(exp[qi]), what + (qi, int(n[qi]), len(exp[qi]))
            got = sorted(tuple(int(x) for x in r) for r in hits[qi, :min(len(exp[qi]), cap)])
            if qi in b.truncated:
                assert set(got) <= set(exp[qi]) and len(set(got)) == cap, what + (qi,)
            else:
                assert got == sorted(exp[qi]), what + (qi,)
        FORM_RUNS["match" if mm <= cases.CONSTANTS["kTop"] else "fixup"].add(cs.name)
        _same_blocks(blk, want, exp, b.truncated, what + ("topk_shard",))
        if fused is not None and not b.truncated:
            assert (blk == fused).all(), what
        # the single-query call (ts_find_fused_kernel, both TOP5 values), once per min_match of the batch
        if mm <= cases.CONSTANTS["kTop"] and b.forms is None and (mm, k, cap) == [r for r in b.runs if r[0] == mm][0]:
            for qi in range(real):
                got = dc.find_duplicates(queries[qi], mm, exclude_id=excl[qi] if excl else -1, with_kth=True)
                assert sorted(got) == sorted(exp[qi]), what + ("find_duplicates", qi)
            FORM_RUNS["find"].add(cs.name)


@pytest.mark.parametrize("name", cases.NAMES)
def test_lookup_case_equals_the_oracle_in_every_form(name):
    cs = cases.case(name)
    dc = tc.DeviceCorpus(0)
    try:
        dc.upload_csr(cs.corpus.ids, cs.corpus.offs, cs.corpus.keys)
        st, bk = dc.index_stats(), dc.bucket_stats()
        assert st["indexed_rows"] == cs.corpus.ids.size and st["delta_rows"] == 0 and st["postings"] == cs.corpus.keys.size
        assert bk["sub_indexes"] == cs.n_sub == cases.n_sub(cs.corpus.ids.size) and (bk["buckets"] > 0) == cs.bucket
        for bi in range(len(cs.batches)):
            _run_batch(dc, cs, 0, cs.corpus, bi)
        if cs.edits:
            replaced, appended = cs.edits
            for r, keys in replaced.items():
                dc.upsert(int(cs.corpus.ids[r]), np.asarray(keys, dtype=np.float64).tolist())
            for vid, keys in appended:
                dc.upsert(int(vid), np.asarray(keys, dtype=np.float64).tolist())
            st = dc.index_stats()
            assert st["delta_rows"] == len(replaced) + len(appended) and st["builds"] == 1      # dead in the index
            after = cases.edited(cs)
            for bi in cs.again:
                _run_batch(dc, cs, 1, after, bi)
    finally:
        dc.close()


def test_every_form_ran_for_every_case_meant_for_it():
    """(runs behind the cases above: a form that silently took another path, or a case that lost a form, fails here)"""
    batched = {n for n in cases.NAMES if not n.startswith("groups")}         # (groups: the unfused lookup only)
    assert FORM_RUNS["block"] == batched and FORM_RUNS["find"] == batched
    assert FORM_RUNS["match"] == set(cases.NAMES)
    assert FORM_RUNS["fused"] == batched                      # (wave_cache_sub1: its batches are padded to 2,048 queries)
    # two queries per block where both fit: not the batches of 512 positions or more
    assert FORM_RUNS["pair"] == batched - {"chunks", "wq_chunks"}
    assert FORM_RUNS["wave"] == batched - {"wave_cache_sub1"}                # every handle of one sub-index
    assert FORM_RUNS["fixup"] == {"modes"}
