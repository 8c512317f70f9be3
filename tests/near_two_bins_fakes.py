"""Test-only stand-ins for Inspector(near_two_bins=True) (never imported by the product): a corpus that records which
of its align_* methods was called with which keywords and answers with one fixed hit, a store around it, and a corpus
whose methods have the signatures from before the option - it must keep working while the option is off."""
import numpy as np

from tests import align_topk_ref as atr

HIT = (42, 400, -30, 20)                    # video_id, row_len, best_bin, votes


class TwoBinsCorpus:
    """answers every search with the one hit HIT (rate index 0, span 3..22, nr 20), or refuses the query"""
    supports_align_wide = supports_align_rates = supports_align_span = supports_align_parts = True

    def __init__(self, refuse=False):
        self.refuse, self.calls = refuse, []

    def _answer(self, name, queries, cols, kw):
        self.calls.append((name, dict(kw)))
        rows = np.zeros((len(queries), kw["k"], cols), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[:, 0] = (HIT + (0, 3, 22, 20))[:cols]
        return rows, np.full(len(queries), atr.REFUSED if self.refuse else 1, dtype=np.int64)

    def align(self, timestamps, eps=0.1, max_offset=60.0):
        self.calls.append(("align", dict(eps=eps, max_offset=max_offset)))
        return np.array([HIT + (0,)], dtype=np.int32)

    def align_topk(self, queries, **kw):
        return self._answer("align_topk", queries, 4, kw)

    def align_wide_topk(self, queries, **kw):
        return self._answer("align_wide_topk", queries, 4, kw)

    def align_rates_topk(self, queries, **kw):
        return self._answer("align_rates_topk", queries, 5, kw)

    def align_span_topk(self, queries, **kw):
        return self._answer("align_span_topk", queries, 8, kw)

    def align_parts(self, queries, video_ids, **kw):
        raise AssertionError("near_parts and near_two_bins are refused together")


class OldCorpus:
    """the methods as they were before the option: no two_bins keyword anywhere"""
    supports_align_wide = True

    def __init__(self):
        self.calls = []

    def align(self, timestamps, eps=0.1, max_offset=60.0):
        return np.array([HIT + (0,)], dtype=np.int32)

    def _hit(self, name, Q, k):
        self.calls.append(name)
        rows = np.zeros((Q, k, 4), dtype=np.int32)
        rows[:, :, 0] = -1
        rows[:, 0] = HIT
        return rows, np.ones(Q, dtype=np.int64)

    def align_topk(self, queries, *, eps, max_offset, k, min_votes=1, min_score=0, exclude_ids=None, max_query_len=None):
        return self._hit("align_topk", len(queries), k)

    def align_wide_topk(self, queries, *, eps, max_offset=None, k=16, min_votes=1, min_score=0, contain=False,
                        exclude_ids=None, max_query_len=None):
        return self._hit("align_wide_topk", len(queries), k)


class Store:
    def __init__(self, corpus):
        self.corpus = corpus

    def get_video_by_id(self, vid):
        return None


def two_bins_backend(**kw):
    """tests/near_service_fakes.NearServiceBackend + `two_bins` on local_align: the block of tests/align_two_bins_ref.py
    where the keyword is set, the stand-in's own otherwise; `heard` records, per local call, whether the keyword came.
    (A function: the stand-ins it builds on import torch, which the Inspector's tests above do not need.)"""
    import torch

    from tests import align_two_bins_ref as tb
    from tests.near_fakes import _queries
    from tests.near_service_fakes import NearServiceBackend
    from tvidz_amd.corpus import FORM_RATES, FORM_SPAN, FORM_WIDE

    class TwoBinsBackend(NearServiceBackend):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.heard = []

        def local_align(self, form, d_q, d_off, max_len, k, d_excl, **ask):
            self.heard.append((form.stem, "two_bins" in ask))
            if not ask.pop("two_bins", False):
                return super().local_align(form, d_q, d_off, max_len, k, d_excl, **ask)
            name = {FORM_WIDE: "wide", FORM_RATES: "rates", FORM_SPAN: "span"}[form]
            excl = None if d_excl is None else [int(e) for e in d_excl]
            max_offset = ask["max_offset"]
            max_offset = (1 << 22) * float(ask["eps"]) if max_offset is None else float(max_offset)
            block = tb.topk_two_bins_ref(name, self._rows(), _queries(d_q, d_off), ask["eps"], max_offset, k,
                                         rates=tuple(ask.get("rates") or (1.0,)), min_votes=ask["min_votes"],
                                         min_score=ask["min_score"], contain=ask.get("contain", False),
                                         local=ask.get("local", False), exclude_ids=excl, max_query_len=max_len)
            return torch.from_numpy(block.astype(np.int32))

    return TwoBinsBackend(**kw)
