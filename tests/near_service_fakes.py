"""Test-only stand-ins for the searches with rates and spans and for the parts call over a sharded table (never imported
by the product): tests/near_fakes.py's NearBackend, with sharded.HipBackend's local_align / align_merge of the two forms
that carry a rate list and its local_parts / parts_merge answered by the plain-Python restatements -
tests/align_rates_ref.py, tests/align_span_ref.py and tests/align_parts_ref.py."""
import numpy as np
import torch

from tests import align_parts_ref as apr, align_rates_ref as arr, align_span_ref as asr, align_wide_ref as awr
from tests.fakes import CutReader, OracleCorpus, cut_inspector, cuts_of_key
from tests.near_fakes import NearBackend, _queries
from tvidz_amd.corpus import ALIGN_FORMS, FORM_RATES, FORM_SPAN


class RatedBackend(NearBackend):
    """NearBackend + the forms with rates on CPU tensors (`align_forms`: all four unless told), and no parts call.
    `calls` records every local call in order: (what, Q, the parameters that tell two batched calls apart)."""

    def __init__(self, *a, align_forms=ALIGN_FORMS, **kw):
        super().__init__(*a, align_forms=align_forms, **kw)
        self.calls = []

    def _rows(self):
        ids, offs, keys = self._csr()
        return [(int(ids[c]), keys[offs[c]:offs[c + 1]].tolist()) for c in range(len(ids))]

    def local_align(self, form, d_q, d_off, max_len, k, d_excl, *, eps, max_offset, min_votes, min_score, contain=False,
                    local=False, rates=None):
        if form not in (FORM_RATES, FORM_SPAN):
            self.calls.append((form.stem, len(d_off) - 1, (float(eps), max_offset, int(k), int(min_votes), int(min_score), bool(contain))))
            return super().local_align(form, d_q, d_off, max_len, k, d_excl, eps=eps, max_offset=max_offset, min_votes=min_votes,
                                       min_score=min_score, contain=contain)
        queries = _queries(d_q, d_off)
        excl = None if d_excl is None else [int(e) for e in d_excl]
        max_offset = awr.MAX_B * float(eps) if max_offset is None else float(max_offset)
        rates = tuple(float(r) for r in rates)
        self.calls.append((form.stem, len(queries), (float(eps), max_offset, int(k), int(min_votes), int(min_score), bool(contain),
                                                     bool(local), rates)))
        if form == FORM_RATES:
            block = arr.topk_rates_ref(self._rows(), queries, eps, max_offset, rates, k, min_votes, min_score, contain, excl,
                                       max_query_len=max_len)
        else:
            block = asr.topk_span_ref(self._rows(), queries, eps, max_offset, rates, k, min_votes, min_score, contain, local,
                                      excl, max_query_len=max_len)
        return torch.from_numpy(block.astype(np.int32))

    def align_merge(self, form, gathered, k, d_q, d_off, **flags):
        if form not in (FORM_RATES, FORM_SPAN):
            return super().align_merge(form, gathered, k, d_q, d_off, **flags)
        ref = arr.merge_ref if form == FORM_RATES else asr.merge_ref
        rows, totals = ref(gathered.numpy(), _queries(d_q, d_off), *(flags[n] for n in form.flags))
        return torch.from_numpy(rows.astype(np.int32)), torch.from_numpy(totals.astype(np.int32))


class NearServiceBackend(RatedBackend):
    """RatedBackend + local_parts / parts_merge: everything sharded.HipBackend answers."""

    def local_parts(self, d_q, d_off, max_len, d_ids, *, eps, max_offset=None, rates=(1.0,), min_votes, max_parts):
        queries = _queries(d_q, d_off)
        max_offset = awr.MAX_B * float(eps) if max_offset is None else float(max_offset)
        rates = tuple(float(r) for r in rates)
        ids = d_ids.numpy()
        self.calls.append(("align_parts", len(queries), (float(eps), max_offset, int(ids.shape[1]), int(min_votes), rates,
                                                         int(max_parts))))
        out = apr.align_parts_ref(self._rows(), queries, ids, eps, max_offset, rates, min_votes, max_parts, max_query_len=max_len)
        return torch.from_numpy(out.astype(np.int32))

    def parts_merge(self, gathered):
        return torch.from_numpy(apr.merge_shards_ref(gathered.numpy()).astype(np.int32))


def near_service_rank_parts(rank, world, group, a):
    """service.py `--parts tests.near_service_fakes:near_service_rank_parts`: near_fakes.near_rank_parts with the stand-ins
    of all four forms and of the parts call."""
    from tvidz_amd import service, sharded
    shard = OracleCorpus()
    matcher = sharded.ShardedMatcher(NearServiceBackend(live=shard), k=a.k, cap=max(a.cap, a.k), group=group)
    return dict(shard=shard, matcher=matcher, xdev="cpu",
                inspector=lambda store: cut_inspector(
                    store, device="cuda:0", max_workers=a.workers, **service.near_kwargs(a),
                    frame_source=lambda bucket, key, filename, uid: (CutReader(cuts_of_key(key)), None)))
