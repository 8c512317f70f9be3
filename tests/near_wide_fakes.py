"""Test-only stand-ins for the near-duplicate search at any shift over a sharded table (never imported by the product):
tests/near_fakes.NearBackend with sharded.HipBackend's two wide methods answered by the plain-Python restatements
(tests/align_wide_ref.py for a rank's block, tests/align_wide_shard_ref.py for the merge)."""
import numpy as np
import torch

from tests import align_wide_ref as awr, align_wide_shard_ref as wsr
from tests.fakes import CutReader, OracleCorpus, cut_inspector, cuts_of_key
from tests.near_fakes import NearBackend


def _queries(d_q, d_off):
    q_all, off = d_q.numpy(), d_off.numpy()
    return [q_all[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


class WideBackend(NearBackend):
    """near_fakes.NearBackend + local_align_wide_topk / align_wide_topk_merge on CPU tensors."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.wide_calls = []                # (Q, eps, max_offset, k, min_votes, min_score, contain) of every batch

    def local_align_wide_topk(self, d_q, d_off, max_len, eps, max_offset, k, min_votes, min_score, contain, d_excl):
        queries = _queries(d_q, d_off)
        max_offset = awr.MAX_B * float(eps) if max_offset is None else float(max_offset)
        self.wide_calls.append((len(queries), float(eps), max_offset, int(k), int(min_votes), int(min_score), bool(contain)))
        ids, offs, keys = self._csr()
        rows = [(int(ids[c]), keys[offs[c]:offs[c + 1]].tolist()) for c in range(len(ids))]
        excl = None if d_excl is None else [int(e) for e in d_excl]
        block = awr.topk_wide_ref(rows, queries, eps, max_offset, k, min_votes, min_score, contain, excl,
                                  max_query_len=max_len)
        return torch.from_numpy(block.astype(np.int32))

    def align_wide_topk_merge(self, gathered, k, d_q, d_off, contain):
        rows, totals = wsr.merge_ref(gathered.numpy(), _queries(d_q, d_off), contain)
        return torch.from_numpy(rows.astype(np.int32)), torch.from_numpy(totals.astype(np.int32))


def wide_rank_parts(rank, world, group, a):
    """service.py `--parts tests.near_wide_fakes:wide_rank_parts`: near_fakes.near_rank_parts with the wide stand-ins."""
    from tvidz_amd import service, sharded
    shard = OracleCorpus()
    matcher = sharded.ShardedMatcher(WideBackend(live=shard), k=a.k, cap=max(a.cap, a.k), group=group)
    return dict(shard=shard, matcher=matcher, xdev="cpu",
                inspector=lambda store: cut_inspector(
                    store, device="cuda:0", max_workers=a.workers, **service.near_kwargs(a),
                    frame_source=lambda bucket, key, filename, uid: (CutReader(cuts_of_key(key)), None)))
