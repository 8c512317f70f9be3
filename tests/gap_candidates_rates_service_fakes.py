"""Test-only stand-in for the rates candidates call over a sharded table (never imported by the product):
tests/gap_candidates_service_fakes.py's backend with sharded.HipBackend's local_candidates_rates /
candidates_rates_merge answered by the plain-Python restatements - tests/gap_candidates_rates_ref.py for a rank's block,
tests/gap_candidates_rates_merge_ref.py for the merge."""
import numpy as np
import torch

from tests import gap_candidates_rates_merge_ref as mref, gap_candidates_rates_ref as rr
from tests.gap_candidates_service_fakes import CandidatesBackend
from tests.near_fakes import _queries


class CandidatesRatesBackend(CandidatesBackend):
    """CandidatesBackend + local_candidates_rates / candidates_rates_merge: `calls` gains ("align_candidates_rates", Q,
    (gap_eps, c, min_count, cap, rates)) for every local call."""

    def local_candidates_rates(self, d_q, d_off, max_len, rates, *, c, min_count=2, cap=4096, d_exclude_ids=None):
        queries = _queries(d_q, d_off)
        excl = None if d_exclude_ids is None else [int(e) for e in d_exclude_ids]
        gap_eps = self.live.gap_eps
        rates = tuple(float(r) for r in rates)
        self.calls.append(("align_candidates_rates", len(queries), (float(gap_eps), int(c), int(min_count), int(cap), rates)))
        block = rr.candidates_rates(self._rows(), queries, gap_eps, rates, c, min_count=min_count, cap=cap, exclude_ids=excl,
                                    max_query_len=max_len)
        return torch.from_numpy(np.asarray(block).astype(np.int32))

    def candidates_rates_merge(self, gathered):
        return torch.from_numpy(mref.merge(gathered.numpy()))
