"""Test-only stand-ins for the candidates call over a sharded table (never imported by the product):
tests/near_service_fakes.py's backend with sharded.HipBackend's local_candidates / candidates_merge answered by the
plain-Python restatements - tests/gap_candidates_ref.py for a rank's block, tests/gap_candidates_merge_ref.py for the
merge - and an oracle shard that says which gap width it keeps."""
import numpy as np
import torch

from tests import gap_candidates_merge_ref as mref, gap_candidates_ref as ref
from tests.fakes import OracleCorpus
from tests.near_fakes import _queries
from tests.near_service_fakes import NearServiceBackend


class GapOracleCorpus(OracleCorpus):
    """fakes.OracleCorpus + the gap index's switch: it only remembers the width (the backend reads it)."""

    def __init__(self):
        super().__init__()
        self.gap_eps = 0.0

    def set_gap_index(self, gap_eps):
        self.gap_eps = float(gap_eps)

    def gap_index_stats(self):
        on = self.gap_eps > 0
        return dict(gap_eps=self.gap_eps, rows=len(self.rows) if on else 0, codes=0, indexed_rows=0, delta_rows=0, builds=int(on))


class CandidatesBackend(NearServiceBackend):
    """NearServiceBackend + local_candidates / candidates_merge: `calls` gains ("align_candidates", Q, (gap_eps, c,
    min_count, cap)) for every local call."""

    def local_candidates(self, d_q, d_off, max_len, *, c, min_count=2, cap=4096, d_exclude_ids=None):
        queries = _queries(d_q, d_off)
        excl = None if d_exclude_ids is None else [int(e) for e in d_exclude_ids]
        gap_eps = self.live.gap_eps
        self.calls.append(("align_candidates", len(queries), (float(gap_eps), int(c), int(min_count), int(cap))))
        block = ref.candidates(self._rows(), queries, gap_eps, c, min_count=min_count, cap=cap, exclude_ids=excl,
                               max_query_len=max_len)
        return torch.from_numpy(block.astype(np.int32))

    def candidates_merge(self, gathered):
        return torch.from_numpy(mref.merge(gathered.numpy()))
