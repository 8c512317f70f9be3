"""Device-resident image of the `video_timestamps` table and the matcher over it.

Host side of the seam at /root/reference/inspector/db.py:76-94 (`find_duplicates`) and of the
per-cut loop around it (inspector/app.py:231-255).  All compute is in csrc/tvz_match.hip; this
module only marshals arrays through the C ABI of include/tvz.h.
"""
from __future__ import annotations

import ctypes as C
import threading
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

KTH_NEVER = _lib.KTH_NEVER


def rows_to_csr(rows: Iterable[Tuple[int, Sequence[float]]]):
    """[(video_id, [ts...])] -> (ids int32[C], offsets int64[C+1], keys float64[n])."""
    rows = list(rows)
    ids = np.fromiter((int(v) for v, _ in rows), dtype=np.int32, count=len(rows))
    lens = np.fromiter((len(t) for _, t in rows), dtype=np.int64, count=len(rows))
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    keys = np.empty(int(offs[-1]), dtype=np.float64)
    for (_, t), o, n in zip(rows, offs[:-1], lens):
        if n:
            keys[o:o + n] = np.asarray(t, dtype=np.float64)
    return ids, offs, keys


def _ptr(a: Optional[np.ndarray]):
    return None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)


def workspace_bytes(Q: int, max_query_len: int, cap: int = 0, k: int = 0, n_ranks: int = 1,
                    total_query_keys: int = 0) -> int:
    """tvz_match_workspace_bytes: scratch of the batched calls (k = 0: the hash-join tables only).
    `total_query_keys` (the length of d_queries) matters for a batch that holds queries of more than 4,095
    timestamps: their sorted distinct keys are made on the device in a tail of the workspace
    (tvz_match_workspace_bytes_long)."""
    if max_query_len > 4095 and total_query_keys:
        return int(_lib.load().tvz_match_workspace_bytes_long(int(Q), int(max_query_len), int(cap), int(k),
                                                              int(n_ranks), int(total_query_keys)))
    return int(_lib.load().tvz_match_workspace_bytes(int(Q), int(max_query_len), int(cap), int(k),
                                                     int(n_ranks)))


def tol_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0) -> int:
    """tvz_match_tol_workspace_bytes: scratch of the tolerant batched match (the sorted copy of every query)."""
    return int(_lib.load().tvz_match_tol_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys)))


def tol_topk_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16,
                             n_ranks: int = 1) -> int:
    """tvz_match_tol_topk_workspace_bytes: the sorted queries, one kept list of k words per sweep block, the local
    block and `n_ranks` gathered ones - nothing in it grows with the number of hits."""
    return int(_lib.load().tvz_match_tol_topk_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys),
                                                              int(k), int(n_ranks)))


@dataclass(frozen=True)
class AlignForm:
    """One form of the alignment top-k as the wrappers below see it; what the form is to the library is said in one
    place too (csrc/tvz_match.hip, kAlignForms).  A form is declared here once; the public align_* functions of this
    module, of DeviceCorpus and of Comm are forwards that name theirs."""
    stem: str                   # the library's tvz_<stem>, tvz_<stem>_workspace_bytes, tvz_<stem>_merge, tvz_<stem>_shards, ..
    cols: int                   # int32 columns of a row
    widest: bool                # max_offset=None means ALIGN_WIDE_MAX_B x eps
    rates: bool                 # a rate list is passed
    flags: Tuple[str, ...]      # which of contain / local exist: () has no flags argument at all.  The score kinds: what
    #                             a form's merge is told too
    two_bins: bool = False      # its calls take `two_bins` (TVZ_ALIGN_TWO_BINS); its merge accepts the bit and ignores it

    def fn(self, suffix: str = ""):
        return getattr(_lib.load(), "tvz_" + self.stem + suffix)

    @property
    def rccl(self) -> bool:
        """Does the library have the form's RCCL call, tvz_<stem>_sharded (Comm.align_sharded)?"""
        return "tvz_" + self.stem + "_sharded" in _lib.SIGNATURES


FORM_BOUNDED = AlignForm("align_topk", 4, False, False, ())
FORM_WIDE = AlignForm("align_wide_topk", 4, True, False, ("contain",), True)
FORM_RATES = AlignForm("align_rates_topk", 5, True, True, ("contain",), True)
FORM_SPAN = AlignForm("align_span_topk", 8, True, True, ("contain", "local"), True)
ALIGN_FORMS = (FORM_BOUNDED, FORM_WIDE, FORM_RATES, FORM_SPAN)


def _align_args(f: AlignForm, eps, max_offset, min_votes, min_score, rates=None, contain=False, local=False,
                two_bins=False) -> list:
    """What a form's call, its _shards and its _sharded take between max_query_len and the exclusions, in the ABI's
    order: eps, max_offset, [h_rates, n_rates,] min_votes, min_score, [flags]."""
    a = [float(eps), _wide_offset(eps, max_offset) if f.widest else float(max_offset)]
    if f.rates:
        a += _rates(rates)
    return a + [int(min_votes), int(min_score)] + _align_flags(f, contain, local, two_bins)


def _align_flags(f: AlignForm, contain=False, local=False, two_bins=False) -> list:
    """The flags argument of a form's calls and of its merge: none at all for the form without flags."""
    if two_bins and not f.two_bins:
        raise ValueError(f"tvz_{f.stem} has no TVZ_ALIGN_TWO_BINS")
    return [_span_flags(contain, local, two_bins)] if f.flags else []


def form_workspace_bytes(f: AlignForm, Q: int, max_query_len: int, total_query_keys: int, k: int,
                         n_ranks: Optional[int] = None) -> int:
    """tvz_<stem>_workspace_bytes, or with `n_ranks` tvz_<stem>_sharded_workspace_bytes of a form that has one."""
    if n_ranks is None:
        return int(f.fn("_workspace_bytes")(int(Q), int(max_query_len), int(total_query_keys), int(k)))
    return int(f.fn("_sharded_workspace_bytes")(int(Q), int(max_query_len), int(total_query_keys), int(k), int(n_ranks)))


def align_topk_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16) -> int:
    """tvz_align_topk_workspace_bytes: the sorted queries, the hit totals and one kept list per sweep block - nothing
    in it grows with rows or hits."""
    return form_workspace_bytes(FORM_BOUNDED, Q, max_query_len, total_query_keys, k)


def align_topk_sharded_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16,
                                       n_ranks: int = 1) -> int:
    """tvz_align_topk_sharded_workspace_bytes: align_topk_workspace_bytes + the local block and `n_ranks` gathered ones
    (Q x (k + 1) x 16 bytes each)."""
    return form_workspace_bytes(FORM_BOUNDED, Q, max_query_len, total_query_keys, k, n_ranks)


ALIGN_SCORE_ONE = 1 << 20
ALIGN_TOPK_MAX_LEN = 4095                   # include/tvz.h: the batched calls take queries of up to 4095 timestamps
ALIGN_TOPK_MAX_K, ALIGN_TOPK_MAX_BINS = 64, 4096     # include/tvz.h, tvz_align_topk: rows kept per query, offset bins
ALIGN_REFUSED = -(1 << 31)                  # a query's total when tvz_align_topk refused it (INT32_MIN)


def align_score(votes: int, nv: int, row_len: int) -> int:
    """The score tvz_align_topk orders by: the tolerant Jaccard v / (nv + row_len - v), v = min(votes, nv, row_len), in
    20-bit fixed point, floor((v << 20) / u) - exact integer arithmetic, 0..2^20 (0 where nothing can match)."""
    v = min(int(votes), int(nv), int(row_len))
    u = int(nv) + int(row_len) - v
    return (v << 20) // u if u > 0 else 0


def align_order_key(row, nv: int):
    """Sort key of one (video_id, row_len, best_bin, votes) hit of a query with nv non-NaN values: the order
    tvz_align_topk keeps its rows in (better score, smaller video id, bin, then row_len and votes)."""
    vid, row_len, best_bin, votes = (int(x) for x in row)
    return (-align_score(votes, nv, row_len), vid, best_bin, row_len, votes)


def align_wide_topk_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16) -> int:
    """tvz_align_wide_topk_workspace_bytes: as align_topk_workspace_bytes, with 20 bytes per kept hit instead of 16."""
    return form_workspace_bytes(FORM_WIDE, Q, max_query_len, total_query_keys, k)


def align_wide_topk_sharded_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16,
                                            n_ranks: int = 1) -> int:
    """tvz_align_wide_topk_sharded_workspace_bytes: align_wide_topk_workspace_bytes + the local block and `n_ranks`
    gathered ones (Q x (k + 1) x 16 bytes each)."""
    return form_workspace_bytes(FORM_WIDE, Q, max_query_len, total_query_keys, k, n_ranks)


ALIGN_WIDE_MAX_B = 1 << 22                  # include/tvz.h TVZ_ALIGN_WIDE_MAX_B: tvz_align_wide_topk's bins per side
ALIGN_CONTAIN = 1                           # include/tvz.h TVZ_ALIGN_CONTAIN
ALIGN_TWO_BINS = 8                          # include/tvz.h TVZ_ALIGN_TWO_BINS: votes counted over two adjacent bins, best_bin
#                                             the lower one (4 is no flag).  `two_bins=True` of the wide, rates and span calls


def align_containment(votes: int, nv: int, row_len: int) -> int:
    """The score tvz_align_wide_topk orders by with TVZ_ALIGN_CONTAIN: v / min(nv, row_len), v = min(votes, nv,
    row_len), in 20-bit fixed point - 2^20 when every cut of the shorter side aligns."""
    v = min(int(votes), int(nv), int(row_len))
    u = min(int(nv), int(row_len))
    return (v << 20) // u if u > 0 else 0


def align_wide_order_key(row, nv: int, contain: bool = False):
    """align_order_key for tvz_align_wide_topk: the same tuple, scored by either kind."""
    vid, row_len, best_bin, votes = (int(x) for x in row)
    score = align_containment if contain else align_score
    return (-score(votes, nv, row_len), vid, best_bin, row_len, votes)


ALIGN_MAX_RATES = 8                         # include/tvz.h TVZ_ALIGN_MAX_RATES: tvz_align_rates_topk's rate list


def align_rates_topk_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16) -> int:
    """tvz_align_rates_topk_workspace_bytes: as align_wide_topk_workspace_bytes, with 24 bytes per kept hit."""
    return form_workspace_bytes(FORM_RATES, Q, max_query_len, total_query_keys, k)


def align_rates_topk_sharded_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16,
                                             n_ranks: int = 1) -> int:
    """tvz_align_rates_topk_sharded_workspace_bytes: align_rates_topk_workspace_bytes + the local block and `n_ranks`
    gathered ones (Q x (k + 1) x 20 bytes each)."""
    return form_workspace_bytes(FORM_RATES, Q, max_query_len, total_query_keys, k, n_ranks)


def align_rates_order_key(row, nv: int, contain: bool = False):
    """Sort key of one (video_id, row_len, best_bin, votes, rate_index) row of tvz_align_rates_topk:
    align_wide_order_key, then the rate's index."""
    return align_wide_order_key(row[:4], nv, contain) + (int(row[4]),)


ALIGN_LOCAL = 2                             # include/tvz.h TVZ_ALIGN_LOCAL: tvz_align_span_topk's score inside the span


def align_span_topk_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16) -> int:
    """tvz_align_span_topk_workspace_bytes: as align_wide_topk_workspace_bytes, with 32 bytes per kept hit."""
    return form_workspace_bytes(FORM_SPAN, Q, max_query_len, total_query_keys, k)


def align_span_topk_sharded_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16,
                                            n_ranks: int = 1) -> int:
    """tvz_align_span_topk_sharded_workspace_bytes: align_span_topk_workspace_bytes + the local block and `n_ranks`
    gathered ones (Q x (k + 1) x 32 bytes each)."""
    return form_workspace_bytes(FORM_SPAN, Q, max_query_len, total_query_keys, k, n_ranks)


def align_local_score(votes: int, nq: int, nr: int) -> int:
    """The score tvz_align_span_topk orders by with TVZ_ALIGN_LOCAL: the Jaccard of the two sides inside the span, v /
    (nq + nr - v) with v = min(votes, nq, nr), in 20-bit fixed point; 0 where a side is empty."""
    nq, nr = int(nq), int(nr)
    if nq <= 0 or nr <= 0:
        return 0
    v = min(int(votes), nq, nr)
    return (v << 20) // (nq + nr - v)


def align_span_order_key(row, nv: int, contain: bool = False, local: bool = False):
    """Sort key of one (video_id, row_len, best_bin, votes, rate_index, t_first, t_last, nr) row of
    tvz_align_span_topk: align_rates_order_key - scored inside the span with `local` - then the three span fields."""
    vid, row_len, best_bin, votes, rate, t_first, t_last, nr = (int(x) for x in row)
    if contain and local:
        raise ValueError("contain and local are two score kinds: one of them")
    if local:
        head = (-align_local_score(votes, t_last - t_first + 1, nr), vid, best_bin, row_len, votes, rate)
    else:
        head = align_rates_order_key(row[:5], nv, contain)
    return head + (t_first, t_last, nr)


def _span_flags(contain: bool, local: bool, two_bins: bool = False) -> int:
    return (ALIGN_CONTAIN if contain else 0) | (ALIGN_LOCAL if local else 0) | (ALIGN_TWO_BINS if two_bins else 0)


ALIGN_MAX_PARTS, ALIGN_PARTS_MAX_ROWS = 4, 8     # include/tvz.h TVZ_ALIGN_MAX_PARTS, TVZ_ALIGN_PARTS_MAX_ROWS


def align_parts_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16,
                                max_parts: int = ALIGN_MAX_PARTS) -> int:
    """tvz_align_parts_workspace_bytes: the sorted queries and, per (query, id) pair, the count of rows that carry the
    id, eight candidate rows and every candidate's (1 + max_parts) x 6 words."""
    return int(_lib.load().tvz_align_parts_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys), int(k),
                                                           int(max_parts)))


def align_parts_sharded_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, k: int = 16,
                                        max_parts: int = ALIGN_MAX_PARTS, n_ranks: int = 1) -> int:
    """tvz_align_parts_sharded_workspace_bytes: align_parts_workspace_bytes + the local answer and `n_ranks` gathered
    ones (Q x k x (1 + max_parts) x 24 bytes each)."""
    return int(_lib.load().tvz_align_parts_sharded_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys),
                                                                   int(k), int(max_parts), int(n_ranks)))


ALIGN_CANDIDATES_MAX_C, ALIGN_CANDIDATES_MAX_PROBES = 64, 4095     # include/tvz_gap.h TVZ_GAP_MAX_C, TVZ_GAP_MAX_PROBES
ALIGN_CANDIDATES_REFUSED = -(1 << 31)                               # n_candidates of a refused query


def align_candidates_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, cap: int = 4096,
                                     c: int = 16) -> int:
    """tvz_align_candidates_workspace_bytes: the lookup's hit lists (Q x cap x 12 bytes) and its own workspace, then per
    query value the sorted copy and eight probe slots (76 bytes)."""
    return int(_lib.load().tvz_align_candidates_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys),
                                                                int(cap), int(c)))


def align_candidates_rates_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, n_rates: int = 1,
                                           cap: int = 4096, c: int = 16) -> int:
    """tvz_align_candidates_rates_workspace_bytes: the lookup's hit lists for Q x n_rates probe lists (cap x 12 bytes
    each) and its own workspace, then per query value the sorted copy and eight probe slots per rate (12 + 64 n_rates
    bytes).  0 for arguments the call refuses."""
    return int(_lib.load().tvz_align_candidates_rates_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys),
                                                                      int(n_rates), int(cap), int(c)))


# include/tvz_gap_long.h TVZ_GAP_LONG_SEG_POSITIONS, TVZ_GAP_LONG_MAX_LEN, TVZ_GAP_LONG_LDS_ENTRIES
ALIGN_CANDIDATES_LONG_SEG_POSITIONS, ALIGN_CANDIDATES_LONG_MAX_LEN, ALIGN_CANDIDATES_LONG_LDS_ENTRIES = 511, 4095, 2048


def align_candidates_long_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, cap: int = 4096,
                                          c: int = 16) -> int:
    """tvz_align_candidates_long_workspace_bytes: align_candidates_workspace_bytes with a hit list per SEGMENT of 511
    positions of the longest query (Q x S x cap x 12 bytes) and, where S x cap is above 2,048, per query the fold's table
    (8 bytes x the next power of two at or above 2 x S x cap).  0 for arguments the call refuses."""
    return int(_lib.load().tvz_align_candidates_long_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys),
                                                                     int(cap), int(c)))


ALIGN_CANDIDATES_MERGE_MAX_LISTS = 16                               # include/tvz_gap_shards.h TVZ_GAP_MERGE_MAX_LISTS


def align_candidates_sharded_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, cap: int = 4096,
                                             c: int = 16, n_ranks: int = 1) -> int:
    """tvz_align_candidates_sharded_workspace_bytes: align_candidates_workspace_bytes + the rank's own block and
    `n_ranks` gathered ones (Q x (c + 1) x 8 bytes each)."""
    return int(_lib.load().tvz_align_candidates_sharded_workspace_bytes(int(Q), int(max_query_len), int(total_query_keys),
                                                                        int(cap), int(c), int(n_ranks)))


def align_candidates_merge(blocks: np.ndarray) -> np.ndarray:
    """The blocks of R shards to one align_candidates call, on the host: int32 [R, Q, c + 1, 2] -> int32 [Q, c + 1, 2]
    (include/tvz_gap_shards.h, THE MERGE).  Per query every row with video_id >= 0 takes part, the c largest by (count
    descending, video_id ascending) are kept - equal rows all of them - and padded with (-1, 0); the last row is (-1,
    total): the sum of the shards' |total|, saturated at 2^31 - 1, negated if one was negative, and a query some shard
    refused (ALIGN_CANDIDATES_REFUSED) is refused.  Any R: the rule is associative."""
    blocks = np.asarray(blocks, dtype=np.int32)
    R, Q, c1, _ = blocks.shape
    c = c1 - 1
    out = np.empty((Q, c1, 2), dtype=np.int32)
    out[:, :c, 0], out[:, :c, 1] = -1, 0
    rows = blocks[:, :, :c].transpose(1, 0, 2, 3).reshape(Q, R * c, 2).astype(np.int64)
    valid = rows[:, :, 0] >= 0
    # one sortable word per row, as the kernels': padding sorts last
    word = np.where(valid, (rows[:, :, 1] << 32) | ((1 << 31) - 1 - rows[:, :, 0]), -1)
    order = np.argsort(-word, axis=1, kind="stable")[:, :c]
    best = np.take_along_axis(rows, order[:, :, None], 1)
    keep = np.take_along_axis(valid, order, 1)
    out[:, :c][keep] = best[keep].astype(np.int32)
    t = blocks[:, :, c, 1].astype(np.int64)
    total = np.minimum(np.abs(t).sum(0), (1 << 31) - 1)
    total = np.where((t < 0).any(0), -total, total)
    refused = (t == ALIGN_CANDIDATES_REFUSED).any(0)
    out[refused, :c] = (-1, 0)
    out[:, c, 0] = -1
    out[:, c, 1] = np.where(refused, ALIGN_CANDIDATES_REFUSED, total).astype(np.int32)
    return out


def align_candidates_merge_device(gathered: torch.Tensor, stream: Optional[torch.cuda.Stream] = None,
                                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tvz_align_candidates_merge: align_candidates_merge on the device - the blocks of R <= 16 shards to one
    align_candidates call, int32 [R, Q, c + 1, 2] -> int32 [Q, c + 1, 2], one launch on `stream` (default: the
    current one)."""
    if gathered.dim() != 4 or gathered.shape[3] != 2 or gathered.dtype != torch.int32 or gathered.device.type != "cuda" \
            or not gathered.is_contiguous():
        raise RuntimeError("gathered must be a contiguous int32 CUDA tensor [R, Q, c + 1, 2]")
    R, Q, c1, _ = gathered.shape
    out = _out(out, (Q, c1, 2), gathered.device)
    s = stream if stream is not None else torch.cuda.current_stream(gathered.device)
    with torch.cuda.device(gathered.device):
        _lib.check(_lib.load().tvz_align_candidates_merge(gathered.data_ptr() if gathered.numel() else None, R, Q, c1 - 1,
                                                          out.data_ptr() if out.numel() else None, s.cuda_stream))
    return out


def align_candidates_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                            max_query_len: int, *, c: int, min_count: int = 2, cap: int = 4096,
                            d_exclude_ids: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                            stream: Optional[torch.cuda.Stream] = None):
    """tvz_align_candidates on every handle of ONE device + the merge behind one library call
    (tvz_align_candidates_shards): -> (blocks int32 [R, Q, c + 1, 2], merged int32 [Q, c + 1, 2]).  `workspace`:
    align_candidates_workspace_bytes, one handle's, serves all of them."""
    Q = d_q_offsets.numel() - 1
    dev, s, ws, excl = shards[0]._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                          align_candidates_workspace_bytes(Q, max_query_len, d_queries.numel(), cap, c))
    R = len(shards)
    handles = (C.c_void_p * R)(*[sh._h for sh in shards])
    blocks = torch.empty((R, Q, max(int(c), 0) + 1, 2), dtype=torch.int32, device=dev)
    merged = torch.empty((Q, max(int(c), 0) + 1, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tvz_align_candidates_shards(
            handles, R, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), int(min_count), excl, int(cap),
            int(c), blocks.data_ptr(), merged.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
    return blocks, merged


ALIGN_CANDIDATES_RATES_MERGE_MAX_LISTS = 16          # include/tvz_gap_rates_shards.h TVZ_GAP_RATES_MERGE_MAX_LISTS


def align_candidates_rates_sharded_workspace_bytes(Q: int, max_query_len: int, total_query_keys: int = 0, n_rates: int = 1,
                                                   cap: int = 4096, c: int = 16, n_ranks: int = 1) -> int:
    """tvz_align_candidates_rates_sharded_workspace_bytes: align_candidates_rates_workspace_bytes + the rank's own block
    and `n_ranks` gathered ones (Q x (c + 1) x 12 bytes each)."""
    return int(_lib.load().tvz_align_candidates_rates_sharded_workspace_bytes(
        int(Q), int(max_query_len), int(total_query_keys), int(n_rates), int(cap), int(c), int(n_ranks)))


def align_candidates_rates_merge(blocks: np.ndarray) -> np.ndarray:
    """The blocks of R shards to one align_candidates_rates call, on the host: int32 [R, Q, c + 1, 3] -> int32 [Q, c + 1,
    3] (include/tvz_gap_rates_shards.h, THE MERGE).  Per query every row with video_id >= 0 takes part; per id the
    largest best and the smallest rate index that reaches it - an id appears ONCE; the c largest by (best descending,
    video_id ascending) are kept and padded with (-1, 0, 0); the last row is (-1, total, 0) by align_candidates_merge's
    totals rule.  The lists need not be sorted.  Any R: the rule is associative."""
    blocks = np.asarray(blocks, dtype=np.int32)
    R, Q, c1, _ = blocks.shape
    c = c1 - 1
    out = np.zeros((Q, c1, 3), dtype=np.int32)
    out[:, :, 0] = -1
    rows = blocks[:, :, :c].transpose(1, 0, 2, 3).reshape(Q, R * c, 3).astype(np.int64)
    # by id: id ascending, best descending, rate ascending - the first row of an id is the one that stays
    pad = np.int64((1 << 63) - 1)                             # above every word (an id is below 2^31)
    by_id = np.where(rows[:, :, 0] >= 0, (rows[:, :, 0] << 32) | ((4095 - rows[:, :, 1]) << 4) | rows[:, :, 2], pad)
    by_id = np.sort(by_id, axis=1)
    first = np.ones_like(by_id, dtype=bool)
    first[:, 1:] = (by_id[:, 1:] >> 32) != (by_id[:, :-1] >> 32)
    live = first & (by_id != pad)
    # by output: best descending, id ascending
    word = np.where(live, (((by_id >> 4) & 4095) << 35) | ((by_id >> 32) << 4) | (by_id & 15), pad)
    word = np.sort(word, axis=1)[:, :c]
    keep = word != pad
    n = word.shape[1]
    out[:, :n, 0] = np.where(keep, (word >> 4) & 0x7fffffff, -1)
    out[:, :n, 1] = np.where(keep, 4095 - (word >> 35), 0)
    out[:, :n, 2] = np.where(keep, word & 15, 0)
    t = blocks[:, :, c, 1].astype(np.int64)
    total = np.minimum(np.abs(t).sum(0), (1 << 31) - 1)
    total = np.where((t < 0).any(0), np.where(total == 0, ALIGN_CANDIDATES_REFUSED, -total), total)
    refused = (t == ALIGN_CANDIDATES_REFUSED).any(0)
    out[refused, :c] = (-1, 0, 0)
    out[:, c, 1] = np.where(refused, ALIGN_CANDIDATES_REFUSED, total).astype(np.int32)
    return out


def align_candidates_rates_merge_device(gathered: torch.Tensor, stream: Optional[torch.cuda.Stream] = None,
                                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tvz_align_candidates_rates_merge: align_candidates_rates_merge on the device - the blocks of R <= 16 shards to one
    align_candidates_rates call, int32 [R, Q, c + 1, 3] -> int32 [Q, c + 1, 3], one launch on `stream` (default: the
    current one)."""
    if gathered.dim() != 4 or gathered.shape[3] != 3 or gathered.dtype != torch.int32 or gathered.device.type != "cuda" \
            or not gathered.is_contiguous():
        raise RuntimeError("gathered must be a contiguous int32 CUDA tensor [R, Q, c + 1, 3]")
    R, Q, c1, _ = gathered.shape
    out = _out(out, (Q, c1, 3), gathered.device)
    s = stream if stream is not None else torch.cuda.current_stream(gathered.device)
    with torch.cuda.device(gathered.device):
        _lib.check(_lib.load().tvz_align_candidates_rates_merge(gathered.data_ptr() if gathered.numel() else None, R, Q, c1 - 1,
                                                                out.data_ptr() if out.numel() else None, s.cuda_stream))
    return out


def align_candidates_rates_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                                  max_query_len: int, rates: Sequence[float], *, c: int, min_count: int = 2, cap: int = 4096,
                                  d_exclude_ids: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                  stream: Optional[torch.cuda.Stream] = None):
    """tvz_align_candidates_rates on every handle of ONE device + the merge behind one library call
    (tvz_align_candidates_rates_shards): -> (blocks int32 [R, Q, c + 1, 3], merged int32 [Q, c + 1, 3]).  `workspace`:
    align_candidates_rates_workspace_bytes, one handle's, serves all of them."""
    Q = d_q_offsets.numel() - 1
    h_rates, n_rates = _rates(rates)
    dev, s, ws, excl = shards[0]._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                          align_candidates_rates_workspace_bytes(Q, max_query_len, d_queries.numel(), n_rates,
                                                                                 cap, c))
    R = len(shards)
    handles = (C.c_void_p * R)(*[sh._h for sh in shards])
    blocks = torch.empty((R, Q, max(int(c), 0) + 1, 3), dtype=torch.int32, device=dev)
    merged = torch.empty((Q, max(int(c), 0) + 1, 3), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tvz_align_candidates_rates_shards(
            handles, R, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), h_rates, n_rates, int(min_count),
            excl, int(cap), int(c), blocks.data_ptr(), merged.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
    return blocks, merged


def align_parts_ids(video_ids, Q: int, dev) -> torch.Tensor:
    """The ids of tvz_align_parts as a 2-D int32 tensor [Q, k] on `dev`: a device tensor (any strides) as it is, host
    lists or arrays copied once."""
    if torch.is_tensor(video_ids):
        return video_ids
    a = np.asarray(video_ids, dtype=np.int32)
    if Q == 0 and a.ndim != 2:
        a = np.zeros((0, 1), dtype=np.int32)                # no query: k is of no account
    if a.ndim != 2 or a.shape[0] != Q:
        raise RuntimeError(f"video_ids must be [{Q}][k] ids, one list of k per query")
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def align_parts_merge(answers: np.ndarray) -> np.ndarray:
    """The answers of R shards to one align_parts call, on the host: int32 [R, Q, k, 1 + P, 6] -> int32 [Q, k, 1 + P,
    6].  Per pair, among the shards that hold a row of the id, the answer with the most part-0 votes, the lower shard
    on a tie (shard 0's where none holds one); n_rows is summed; a pair some shard refused stays refused.  Q x k
    blocks of at most 120 bytes per shard: host arithmetic behind the one copy back."""
    R = answers.shape[0]
    n_rows = answers[:, :, :, 0, 4].astype(np.int64)
    votes = answers[:, :, :, 1, 1].astype(np.int64)
    key = np.where(n_rows > 0, votes + 1, 0) * R + (R - 1 - np.arange(R, dtype=np.int64).reshape(R, 1, 1))
    best = key.argmax(0)[None, :, :, None, None]
    out = np.take_along_axis(answers, best, 0)[0].copy()
    out[:, :, 0, 4] = np.minimum(n_rows.sum(0), (1 << 31) - 1)
    refused = (answers[:, :, :, 0, 3] == ALIGN_REFUSED).any(0)
    out[refused, 1:] = 0
    out[refused, 0, 1:3] = 0
    out[refused, 0, 3] = ALIGN_REFUSED
    return out


def align_parts_merge_device(gathered: torch.Tensor, stream: Optional[torch.cuda.Stream] = None,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tvz_align_parts_merge: align_parts_merge on the device - the answers of R <= 16 shards to one align_parts call,
    int32 [R, Q, k, 1 + P, 6] -> int32 [Q, k, 1 + P, 6], one launch on `stream` (default: the current one)."""
    if gathered.dim() != 5 or gathered.shape[4] != 6 or gathered.dtype != torch.int32 or gathered.device.type != "cuda" \
            or not gathered.is_contiguous():
        raise RuntimeError("gathered must be a contiguous int32 CUDA tensor [R, Q, k, 1 + max_parts, 6]")
    R, Q, k, rows, _ = gathered.shape
    out = _out(out, (Q, k, rows, 6), gathered.device)
    s = stream if stream is not None else torch.cuda.current_stream(gathered.device)
    with torch.cuda.device(gathered.device):
        _lib.check(_lib.load().tvz_align_parts_merge(gathered.data_ptr() if gathered.numel() else None, R, Q, k, rows - 1,
                                                     out.data_ptr() if out.numel() else None, s.cuda_stream))
    return out


def _parts_ids(d_video_ids: torch.Tensor, Q: int, d_queries: torch.Tensor):
    """The ids of a parts call as the library takes them: (pointer or None, id_stride, query_id_stride, k)."""
    if d_video_ids.dim() != 2 or d_video_ids.shape[0] != Q or d_video_ids.dtype != torch.int32 \
            or d_video_ids.device != d_queries.device:
        raise RuntimeError(f"video_ids must be an int32 [{Q}, k] tensor on {d_queries.device}")
    return (d_video_ids.data_ptr() if d_video_ids.numel() else None, int(d_video_ids.stride(1)), int(d_video_ids.stride(0)),
            int(d_video_ids.shape[1]))


def align_parts_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                       max_query_len: int, d_video_ids: torch.Tensor, *, eps: float, max_offset: Optional[float] = None,
                       rates: Sequence[float] = (1.0,), min_votes: int, max_parts: int, workspace: torch.Tensor,
                       stream: Optional[torch.cuda.Stream] = None, two_bins: bool = False):
    """tvz_align_parts on every handle of ONE device + the merge behind one library call (tvz_align_parts_shards): ->
    (blocks int32 [R, Q, k, 1 + max_parts, 6], parts int32 [Q, k, 1 + max_parts, 6]).  `workspace`:
    align_parts_workspace_bytes (its size is the library's to judge, as align_topk_shards').  `two_bins`: the votes
    counted over two adjacent bins, through tvz_align_parts_flags_shards (include/tvz_parts_flags.h)."""
    Q = d_q_offsets.numel() - 1
    dev, s, ws, _ = shards[0]._prelude(d_queries, d_q_offsets, None, stream, workspace, None)
    ids, id_stride, query_id_stride, k = _parts_ids(d_video_ids, Q, d_queries)
    R, P = len(shards), int(max_parts)
    handles = (C.c_void_p * R)(*[sh._h for sh in shards])
    blocks = torch.empty((R, Q, k, 1 + max(P, 0), 6), dtype=torch.int32, device=dev)
    parts = torch.empty((Q, k, 1 + max(P, 0), 6), dtype=torch.int32, device=dev)
    front = (handles, R, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), ids, id_stride, query_id_stride,
             k, float(eps), _wide_offset(eps, max_offset), *_rates(rates), int(min_votes), P)
    back = (blocks.data_ptr(), parts.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream)
    with torch.cuda.device(dev):
        if two_bins:
            _lib.check(_lib.load().tvz_align_parts_flags_shards(*front, ALIGN_TWO_BINS, *back))
        else:
            _lib.check(_lib.load().tvz_align_parts_shards(*front, *back))
    return blocks, parts


def _rates(rates):
    """The rate list of the calls with rates -> (a host double array, its length).  What the list may hold is the
    library's to judge (1..ALIGN_MAX_RATES finite rates > 0)."""
    r = [float(x) for x in rates]
    return (C.c_double * max(len(r), 1))(*r), len(r)


class DeviceCorpus:
    """tvz_corpus handle: rows of (video_id, sorted-unique canonical float64 keys) in HBM."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        self.device = int(device)
        h = C.c_void_p()
        _lib.check(self.lib.tvz_corpus_create(C.byref(h), self.device))
        self._h = h
        self._row_bound = 0                 # upper bound on the row count (sizes the output arrays)
        self._tls = threading.local()

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.tvz_corpus_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- mutation (db.py:43-64 add_timestamps; app.py:325-333 clear-db) ----
    def reserve(self, n_rows: int, n_keys: int) -> None:
        _lib.check(self.lib.tvz_corpus_reserve(self._h, int(n_rows), int(n_keys)))

    def upload_csr(self, ids: np.ndarray, offsets: np.ndarray, keys: np.ndarray) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        keys = np.ascontiguousarray(keys, dtype=np.float64)
        if offsets.size != ids.size + 1:
            raise RuntimeError("offsets must have len(ids)+1 entries")
        _lib.check(self.lib.tvz_corpus_upload(self._h, _ptr(ids), C.c_void_p(offsets.ctypes.data),
                                              _ptr(keys), ids.size, keys.size))
        self._row_bound = int(ids.size)

    def upload(self, rows: Iterable[Tuple[int, Sequence[float]]]) -> None:
        self.upload_csr(*rows_to_csr(rows))

    def upsert(self, video_id: int, timestamps: Sequence[float]) -> None:
        """Stream-ordered on the device: returns without waiting for matches in flight; matches
        enqueued afterwards see the new row (include/tvz.h tvz_corpus_upsert)."""
        k = np.ascontiguousarray(np.asarray(timestamps, dtype=np.float64))
        _lib.check(self.lib.tvz_corpus_upsert(self._h, int(video_id), _ptr(k), k.size))
        self._row_bound += 1                # may over-count (a replaced row): only a size bound

    def clear(self) -> None:
        _lib.check(self.lib.tvz_corpus_clear(self._h))
        self._row_bound = 0

    def build_index(self) -> None:
        """Rebuild the inverted index over the current rows now (upload builds it, and it is rebuilt
        automatically as the delta table fills); waits for matches in flight."""
        _lib.check(self.lib.tvz_corpus_build_index(self._h))

    def index_stats(self) -> dict:
        """indexed_rows / delta_rows / postings / distinct_keys / builds; zeros while there is no index."""
        v = [C.c_int64() for _ in range(5)]
        _lib.check(self.lib.tvz_corpus_index_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("indexed_rows", "delta_rows", "postings", "distinct_keys", "builds"),
                        (int(x.value) for x in v)))

    def bucket_stats(self) -> dict:
        """The bucket directory of a one-sub-index handle (tvz_corpus_bucket_stats): buckets (0: none), keys outside
        their home bucket, the farthest walk, keys with external lists, external postings, sub-indexes."""
        v = (C.c_int64 * 6)()
        _lib.check(self.lib.tvz_corpus_bucket_stats(self._h, v))
        return dict(zip(("buckets", "keys_walked_on", "max_walk", "external_lists", "external_postings", "sub_indexes"),
                        (int(x) for x in v)))

    def index_layout(self) -> dict:
        """What the last build made of the open-addressing directory (tvz_corpus_index_layout): entry_bytes / log2 /
        slice_log2 / partitioned (1: built slice by slice, 0: count and fill over the whole directory), and the same
        with a cell_ prefix for the cell directory; zeros where there is none, and for a bucket directory."""
        v = (C.c_int64 * 8)()
        _lib.check(self.lib.tvz_corpus_index_layout(self._h, v))
        names = ("entry_bytes", "log2", "slice_log2", "partitioned")
        return dict(zip(names + tuple("cell_" + n for n in names), (int(x) for x in v)))

    def set_tol_index(self, cell: float) -> None:
        """tvz_corpus_tol_index: cell > 0 makes every index generation of this handle also carry cell postings of `cell`
        seconds (and builds them now if the handle has an index), which the batched tolerant calls then use for
        tol <= cell; 0 turns them off (the next build drops them).  Results never depend on it."""
        _lib.check(self.lib.tvz_corpus_tol_index(self._h, float(cell)))

    def tol_index_stats(self) -> dict:
        """cell (0.0: no cell postings) / cells / postings / builds that carried cell postings / delta_rows."""
        cell, v = C.c_double(), (C.c_int64 * 4)()
        _lib.check(self.lib.tvz_corpus_tol_index_stats(self._h, C.byref(cell), v))
        return dict(zip(("cell", "cells", "postings", "builds", "delta_rows"), [float(cell.value)] + [int(x) for x in v]))

    def set_gap_index(self, gap_eps: float) -> None:
        """tvz_corpus_gap_index: gap_eps > 0 makes the handle keep the gap codes of its rows (three consecutive gaps
        between cuts, quantised to gap_eps seconds: include/tvz_gap.h) in an index of their own, built now and kept
        current by every later upload / upsert / clear; 0 drops them.  `align_candidates` needs them; nothing else
        depends on them."""
        _lib.check(self.lib.tvz_corpus_gap_index(self._h, float(gap_eps)))

    def gap_index_stats(self) -> dict:
        """gap_eps (0.0: off) / rows / codes / indexed_rows / delta_rows / builds of the code table; zeros while off."""
        eps, v = C.c_double(), (C.c_int64 * 5)()
        _lib.check(self.lib.tvz_corpus_gap_index_stats(self._h, C.byref(eps), v))
        return dict(zip(("gap_eps", "rows", "codes", "indexed_rows", "delta_rows", "builds"),
                        [float(eps.value)] + [int(x) for x in v]))

    def align_candidates(self, queries, *, c: int, min_count: int = 2, cap: int = 4096, exclude_ids=None,
                         max_query_len: Optional[int] = None):
        """tvz_align_candidates, host in / host out: per query the `c` stored videos that share the most gap codes with
        it (set_gap_index first) -> (rows int32 [Q, c, 2] of (video_id, count), count descending then id ascending,
        padded with (-1, 0); totals int32 [Q]: the candidates with count >= min_count, negated when they exceeded
        `cap`, ALIGN_CANDIDATES_REFUSED for a query of more than 514 values).  `queries`, `exclude_ids` as align_topk
        takes them."""
        dev = torch.device("cuda", self.device)
        d_q, d_off, Q, max_query_len, d_ex = align_inputs(queries, exclude_ids, max_query_len, dev)
        ws = thread_workspace(self._tls, align_candidates_workspace_bytes(Q, max_query_len, d_q.numel(), cap, c), dev)
        h = self.align_candidates_block(d_q, d_off, max_query_len, c=c, min_count=min_count, cap=cap, d_exclude_ids=d_ex,
                                        workspace=ws).cpu().numpy()
        return np.ascontiguousarray(h[:, :c]), np.ascontiguousarray(h[:, c, 1])

    def align_candidates_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, c: int,
                               min_count: int = 2, cap: int = 4096, d_exclude_ids: Optional[torch.Tensor] = None,
                               out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_candidates, device in / device out: enqueue Q queries -> the block int32 [Q, c + 1, 2].
        `block[:, :c, 0]` is the strided view of ids that align_parts_block takes."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         align_candidates_workspace_bytes(Q, max_query_len, d_queries.numel(), cap, c))
        out = _out(out, (Q, max(int(c), 0) + 1, 2), dev)
        _lib.check(self.lib.tvz_align_candidates(self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len),
                                                 int(min_count), excl, int(cap), int(c), out.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), s.cuda_stream))
        return out

    supports_align_candidates_long = "tvz_align_candidates_long" in _lib.GAP_LONG_SIGNATURES

    def align_candidates_long(self, queries, *, c: int, min_count: int = 2, cap: int = 4096, exclude_ids=None,
                              max_query_len: Optional[int] = None):
        """tvz_align_candidates_long, host in / host out: align_candidates for uploads of up to 4,095 values - the query is
        looked up in segments of 511 positions and the segments' counts are SUMMED per stored video (min_count and `cap`
        hold per segment) -> (rows int32 [Q, c, 2], totals int32 [Q]) as align_candidates returns them: an id at most
        once per query; totals: the distinct candidate ids, or - negated - the segments' hit counts summed when a
        segment's exceeded `cap`; ALIGN_CANDIDATES_REFUSED for a query longer than max_query_len."""
        dev = torch.device("cuda", self.device)
        d_q, d_off, Q, max_query_len, d_ex = align_inputs(queries, exclude_ids, max_query_len, dev)
        ws = thread_workspace(self._tls, align_candidates_long_workspace_bytes(Q, max_query_len, d_q.numel(), cap, c), dev)
        h = self.align_candidates_long_block(d_q, d_off, max_query_len, c=c, min_count=min_count, cap=cap, d_exclude_ids=d_ex,
                                             workspace=ws).cpu().numpy()
        return np.ascontiguousarray(h[:, :c]), np.ascontiguousarray(h[:, c, 1])

    def align_candidates_long_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, c: int,
                                    min_count: int = 2, cap: int = 4096, d_exclude_ids: Optional[torch.Tensor] = None,
                                    out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_candidates_long, device in / device out: enqueue Q queries -> the block int32 [Q, c + 1, 2], in
        align_candidates_block's layout: it goes to align_parts_block and to align_candidates_merge_device as it is."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         align_candidates_long_workspace_bytes(Q, max_query_len, d_queries.numel(), cap, c))
        out = _out(out, (Q, max(int(c), 0) + 1, 2), dev)
        _lib.check(self.lib.tvz_align_candidates_long(self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q,
                                                      int(max_query_len), int(min_count), excl, int(cap), int(c),
                                                      out.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out

    supports_align_candidate_rates = "tvz_align_candidates_rates" in _lib.GAP_RATE_SIGNATURES

    def align_candidates_rates(self, queries, rates: Sequence[float], *, c: int, min_count: int = 2, cap: int = 4096,
                               exclude_ids=None, max_query_len: Optional[int] = None):
        """tvz_align_candidates_rates, host in / host out: align_candidates for copies played at another speed - the
        upload is probed once per rate of `rates` (1..ALIGN_MAX_RATES finite rates > 0, by preference: stored ~= rate x
        upload + shift) and a stored video is named ONCE, at its best rate -> (ids int32 [Q, c], counts int32 [Q, c],
        rate_indexes int32 [Q, c], totals int32 [Q]): the best count per id descending, then id ascending, padded with
        (-1, 0, 0); totals: the (row, rate) pairs with count >= min_count - an upper bound on the ids, not their count
        -, negated when a rate's list exceeded `cap`, ALIGN_CANDIDATES_REFUSED for a query of more than 514 values."""
        dev = torch.device("cuda", self.device)
        d_q, d_off, Q, max_query_len, d_ex = align_inputs(queries, exclude_ids, max_query_len, dev)
        need = align_candidates_rates_workspace_bytes(Q, max_query_len, d_q.numel(), len(rates), cap, c)
        ws = thread_workspace(self._tls, need, dev)
        h = self.align_candidates_rates_block(d_q, d_off, max_query_len, rates, c=c, min_count=min_count, cap=cap,
                                              d_exclude_ids=d_ex, workspace=ws).cpu().numpy()
        return (np.ascontiguousarray(h[:, :c, 0]), np.ascontiguousarray(h[:, :c, 1]), np.ascontiguousarray(h[:, :c, 2]),
                np.ascontiguousarray(h[:, c, 1]))

    def align_candidates_rates_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int,
                                     rates: Sequence[float], *, c: int, min_count: int = 2, cap: int = 4096,
                                     d_exclude_ids: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                                     stream: Optional[torch.cuda.Stream] = None,
                                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_candidates_rates, device in / device out: enqueue Q queries -> the block int32 [Q, c + 1, 3] of
        (video_id, best, rate_index) rows.  `block[:, :c, 0]` is the strided view of ids that align_parts_block takes,
        with the same `rates`."""
        Q = d_q_offsets.numel() - 1
        h_rates, n_rates = _rates(rates)
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         align_candidates_rates_workspace_bytes(Q, max_query_len, d_queries.numel(), n_rates,
                                                                                cap, c))
        out = _out(out, (Q, max(int(c), 0) + 1, 3), dev)
        _lib.check(self.lib.tvz_align_candidates_rates(self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q,
                                                       int(max_query_len), h_rates, n_rates, int(min_count), excl, int(cap),
                                                       int(c), out.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out

    def stats(self) -> Tuple[int, int, int]:
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.lib.tvz_corpus_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- single query, host in / host out: the db.find_duplicates drop-in ----
    def _out_buffers(self, cap: int):
        b = getattr(self._tls, "buf", None)
        if b is None or b[0].size < cap:
            n = max(cap, 1024)
            b = (np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32),
                 C.c_int64())
            b = b + (C.c_void_p(b[0].ctypes.data), C.c_void_p(b[1].ctypes.data), C.c_void_p(b[2].ctypes.data),
                     C.byref(b[3]))
            self._tls.buf = b
        return b

    # this handle answers tolerant asks (inspector.Inspector(match_tolerance > 0) checks for it)
    supports_tolerance = True

    def find_duplicates(self, new_timestamps: Sequence[float], min_match: int = 5,
                        exclude_id: int = -1, with_kth: bool = False, tolerance: float = 0.0):
        """One kernel launch + one stream synchronisation inside the library (for queries of up to
        4095 timestamps with min_match <= 5); the output arrays are per-thread and reused.
        `tolerance` > 0: the opt-in tolerant match (tvz_find_duplicates_tol, include/tvz.h), NOT the
        reference's exact verdict; exactly 0 makes the exact call."""
        q = np.ascontiguousarray(np.asarray(new_timestamps, dtype=np.float64))
        cap = max(self._row_bound, 1)
        tol = float(tolerance)
        while True:
            ids, cnt, kth, n, p_ids, p_cnt, p_kth, p_n = self._out_buffers(cap)
            if tol == 0.0:
                _lib.check(self.lib.tvz_find_duplicates(self._h, _ptr(q), q.size, int(min_match),
                                                        int(exclude_id), ids.size, p_ids, p_cnt, p_kth, p_n))
            else:
                _lib.check(self.lib.tvz_find_duplicates_tol(self._h, _ptr(q), q.size, tol, int(min_match),
                                                            int(exclude_id), ids.size, p_ids, p_cnt, p_kth, p_n))
            if n.value <= ids.size:
                break
            cap = int(n.value)  # rows were added concurrently: retry with room for all
        m = n.value
        if with_kth:
            return list(zip(ids[:m].tolist(), cnt[:m].tolist(), kth[:m].tolist()))
        return list(zip(ids[:m].tolist(), cnt[:m].tolist()))

    # ---- opt-in alignment score (never the verdict; see include/tvz.h tvz_align) ----
    def align(self, timestamps: Sequence[float], eps: float = 0.1, max_offset: float = 60.0):
        """-> int32 array [n_rows,5]: (video_id, row_len, best_bin, votes, votes_at_zero_shift), one
        entry per row of the table as the kernel saw it.  `votes` counts (query, row) pairs: it can
        exceed min(len(timestamps), row_len) when cuts are closer than eps."""
        dev = torch.device("cuda", self.device)
        q = torch.as_tensor(np.asarray(timestamps, dtype=np.float64)).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        n_rows = C.c_int64(0)
        cap = max(self.stats()[0], 1)
        for _ in range(8):
            out = torch.empty((cap, 5), dtype=torch.int32, device=dev)
            _lib.check(self.lib.tvz_align(self._h, q.data_ptr() if q.numel() else None, q.numel(),
                                          float(eps), float(max_offset), out.data_ptr(), cap,
                                          C.byref(n_rows), stream))
            if n_rows.value <= cap:
                return out[:n_rows.value].cpu().numpy()
            cap = n_rows.value + n_rows.value // 4 + 64     # rows were upserted since stats(): retry with room
        raise RuntimeError("tvz_align: the table kept growing faster than the output was resized")

    def align_topk(self, queries, *, eps: float, max_offset: float, k: int = 16, min_votes: int = 1,
                   min_score: int = 0, exclude_ids=None, max_query_len: Optional[int] = None):
        """tvz_align_topk: the k best-aligned rows of every query of a batch, kept inside the sweep.
        `queries`: a list of timestamp lists, or device tensors (d_queries float64, d_q_offsets int64[Q+1]) as the
        batched match calls take them; `exclude_ids`: None or one video id per query (list or device int32 tensor).
        -> (rows int32[Q, k, 4] of (video_id, row_len, best_bin, votes), padded with (-1, 0, 0, 0); totals int32[Q] =
        the true number of hits, ALIGN_REFUSED for a query longer than max_query_len - default: the longest query,
        at most 4,095), as numpy arrays.  Order: align_order_key.  One device-to-host copy of Q x (k + 1) x 16 bytes."""
        return self._align_host(FORM_BOUNDED, queries, k, exclude_ids, max_query_len, eps=eps, max_offset=max_offset,
                                min_votes=min_votes, min_score=min_score)

    def align_topk_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                         max_offset: float, k: int, min_votes: int = 1, min_score: int = 0,
                         d_exclude_ids: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                         stream: Optional[torch.cuda.Stream] = None,
                         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_topk, device in / device out: enqueue Q queries -> the block int32 [Q, k+1, 4] that the sharded
        forms gather and merge (align_topk_merge)."""
        return self._align_block(FORM_BOUNDED, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, out, stream,
                                 workspace, eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score)

    supports_align_wide = True

    def align_wide_topk(self, queries, *, eps: float, max_offset: Optional[float] = None, k: int = 16, min_votes: int = 1,
                        min_score: int = 0, contain: bool = False, two_bins: bool = False, exclude_ids=None,
                        max_query_len: Optional[int] = None):
        """tvz_align_wide_topk: align_topk at any shift - up to ALIGN_WIDE_MAX_B offset bins on either side of zero
        (`max_offset=None`: ALIGN_WIDE_MAX_B x eps, the widest the library takes).  `contain=True` scores by
        v / min(nv, row_len) (align_containment) instead of the tolerant Jaccard, for the excerpt of a longer video.
        `two_bins=True` (TVZ_ALIGN_TWO_BINS; the calls with rates and spans take it too) counts a row's votes over the
        best window of two adjacent bins - best_bin is then the window's LOWER bin, votes the window's count, the
        shift (best_bin + 0.5) x eps - for the copy whose shift lies near a bin's edge.
        Arguments and (rows, totals) otherwise as align_topk; order: align_wide_order_key."""
        return self._align_host(FORM_WIDE, queries, k, exclude_ids, max_query_len, eps=eps, max_offset=max_offset,
                                min_votes=min_votes, min_score=min_score, contain=contain, two_bins=two_bins)

    def align_wide_topk_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                              max_offset: Optional[float] = None, k: int, min_votes: int = 1, min_score: int = 0,
                              contain: bool = False, two_bins: bool = False, d_exclude_ids: Optional[torch.Tensor] = None,
                              out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_wide_topk, device in / device out: enqueue Q queries -> the block int32 [Q, k+1, 4]."""
        return self._align_block(FORM_WIDE, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, out, stream, workspace,
                                 eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, contain=contain,
                                 two_bins=two_bins)

    def align_rates_topk(self, queries, *, eps: float, rates: Sequence[float], max_offset: Optional[float] = None,
                         k: int = 16, min_votes: int = 1, min_score: int = 0, contain: bool = False,
                         two_bins: bool = False, exclude_ids=None,
                         max_query_len: Optional[int] = None):
        """tvz_align_rates_topk: align_wide_topk for copies played at another speed - every row is aligned once per
        rate of `rates` (1..ALIGN_MAX_RATES finite values > 0, in the order of preference; the query's cuts are scaled:
        stored ~= rate x query + shift) and kept once, at the rate with the most votes.  Arguments otherwise as
        align_wide_topk.  -> (rows int32[Q, k, 5] of (video_id, row_len, best_bin, votes, rate_index), padded with
        (-1, 0, 0, 0, 0); totals int32[Q]); order: align_rates_order_key."""
        return self._align_host(FORM_RATES, queries, k, exclude_ids, max_query_len, eps=eps, max_offset=max_offset,
                                min_votes=min_votes, min_score=min_score, rates=rates, contain=contain, two_bins=two_bins)

    def align_rates_topk_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                               rates: Sequence[float], max_offset: Optional[float] = None, k: int, min_votes: int = 1,
                               min_score: int = 0, contain: bool = False,
                               two_bins: bool = False, d_exclude_ids: Optional[torch.Tensor] = None,
                               out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_rates_topk, device in / device out: enqueue Q queries -> the block int32 [Q, k+1, 5]."""
        return self._align_block(FORM_RATES, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, out, stream, workspace,
                                 eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, rates=rates,
                                 contain=contain, two_bins=two_bins)

    def align_span_topk(self, queries, *, eps: float, rates: Sequence[float] = (1.0,), max_offset: Optional[float] = None,
                        k: int = 16, min_votes: int = 1, min_score: int = 0, contain: bool = False, local: bool = False,
                        two_bins: bool = False,
                        exclude_ids=None, max_query_len: Optional[int] = None):
        """tvz_align_span_topk: align_rates_topk that also says WHERE the best bin's votes lie - (t_first, t_last), the
        first and last voting index of the query's non-NaN values sorted ascending, and nr, the row's keys between the
        smallest and the largest voting key.  `local=True` scores by the Jaccard inside that span (align_local_score)
        and finds the copy that is partial on both sides; min_votes is then what keeps chance pairs out.  -> (rows
        int32[Q, k, 8] of (video_id, row_len, best_bin, votes, rate_index, t_first, t_last, nr), padded with (-1, 0, ..);
        totals int32[Q]); order: align_span_order_key."""
        return self._align_host(FORM_SPAN, queries, k, exclude_ids, max_query_len, eps=eps, max_offset=max_offset,
                                min_votes=min_votes, min_score=min_score, rates=rates, contain=contain, local=local,
                                two_bins=two_bins)

    def align_span_topk_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                              rates: Sequence[float] = (1.0,), max_offset: Optional[float] = None, k: int,
                              min_votes: int = 1, min_score: int = 0, contain: bool = False, local: bool = False,
                              two_bins: bool = False,
                              d_exclude_ids: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                              stream: Optional[torch.cuda.Stream] = None,
                              workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_span_topk, device in / device out: enqueue Q queries -> the block int32 [Q, k+1, 8]."""
        return self._align_block(FORM_SPAN, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, out, stream, workspace,
                                 eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, rates=rates,
                                 contain=contain, local=local, two_bins=two_bins)

    def align_parts(self, queries, video_ids, *, eps: float, max_offset: Optional[float] = None,
                    rates: Sequence[float] = (1.0,), min_votes: int, max_parts: int,
                    max_query_len: Optional[int] = None, two_bins: bool = False):
        """tvz_align_parts: EVERY aligned part of named stored videos - the refinement behind a search, for the copy
        with a part put in or taken out, which aligns at two shifts.  `queries` as align_topk takes them; `video_ids`:
        up to k stored video ids per query as an int32 [Q][k] array (list, numpy, device tensor) or any strided 2-D
        view of a device int32 tensor - `block[:, :k, 0]` of a span block is passed with its strides, no copy; -1 is
        no pair.  Every pair is aligned in full at the best of `rates` and up to `max_parts` (1..ALIGN_MAX_PARTS)
        disjoint parts of at least `min_votes` votes are reported.  -> int32 [Q, k, 1 + max_parts, 6] as a numpy
        array: row 0 (video_id, row_len, rate_index, n_parts, n_rows, m), then per part (bin, votes, t_first, t_last,
        nq, nr), zeros beyond n_parts; n_parts = ALIGN_REFUSED marks a refused pair (include/tvz.h).
        `two_bins=True` (tvz_align_parts_flags with TVZ_ALIGN_TWO_BINS, include/tvz_parts_flags.h): every part is the
        best window of two adjacent bins - bin = the lower one, votes = both bins', shift = (bin + 0.5) x eps."""
        dev = torch.device("cuda", self.device)
        d_q, d_off, Q, max_query_len, _ = align_inputs(queries, None, max_query_len, dev)
        d_ids = align_parts_ids(video_ids, Q, dev)
        ws = thread_workspace(self._tls, align_parts_workspace_bytes(Q, max_query_len, d_q.numel(), d_ids.shape[1], max_parts),
                              dev)
        return self.align_parts_block(d_q, d_off, max_query_len, d_ids, eps=eps, max_offset=max_offset, rates=rates,
                                      min_votes=min_votes, max_parts=max_parts, workspace=ws,
                                      **({"two_bins": True} if two_bins else {})).cpu().numpy()

    def align_parts_block(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int,
                          d_video_ids: torch.Tensor, *, eps: float, max_offset: Optional[float] = None,
                          rates: Sequence[float] = (1.0,), min_votes: int, max_parts: int,
                          out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                          workspace: Optional[torch.Tensor] = None, two_bins: bool = False) -> torch.Tensor:
        """tvz_align_parts, device in / device out: enqueue Q x k pairs -> int32 [Q, k, 1 + max_parts, 6].
        `d_video_ids`: a 2-D int32 view [Q, k] on this device, of any strides.  `two_bins`: tvz_align_parts_flags with
        TVZ_ALIGN_TWO_BINS; False calls tvz_align_parts itself."""
        Q = d_q_offsets.numel() - 1
        ids, id_stride, query_id_stride, k = _parts_ids(d_video_ids, Q, d_queries)
        P = int(max_parts)
        dev, s, ws, _ = self._prelude(d_queries, d_q_offsets, None, stream, workspace,
                                      align_parts_workspace_bytes(Q, max_query_len, d_queries.numel(), k, P))
        out = _out(out, (Q, k, 1 + max(P, 0), 6), dev)
        front = (self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), ids, id_stride, query_id_stride,
                 k, float(eps), _wide_offset(eps, max_offset), *_rates(rates), int(min_votes), P)
        back = (out.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream)
        if two_bins:
            _lib.check(self.lib.tvz_align_parts_flags(*front, ALIGN_TWO_BINS, *back))
        else:
            _lib.check(self.lib.tvz_align_parts(*front, *back))
        return out

    supports_align_parts_two_bins = "tvz_align_parts_flags" in _lib.PARTS_FLAGS_SIGNATURES

    def _align_host(self, f: AlignForm, queries, k, exclude_ids, max_query_len, **ask):
        """Any form, host in / host out: the inputs, the calling thread's workspace, the block call, ONE copy back,
        the split into (rows [Q, k, cols], totals [Q])."""
        dev = torch.device("cuda", self.device)
        d_q, d_off, Q, max_query_len, d_ex = align_inputs(queries, exclude_ids, max_query_len, dev)
        ws = thread_workspace(self._tls, form_workspace_bytes(f, Q, max_query_len, d_q.numel(), k), dev)
        h = self._align_block(f, d_q, d_off, max_query_len, k, d_ex, None, None, ws, **ask).cpu().numpy()
        return np.ascontiguousarray(h[:, :k]), np.ascontiguousarray(h[:, k, 1])

    def _align_block(self, f: AlignForm, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, out, stream, workspace,
                     **ask):
        """Any form, device in / device out: the prelude, the block int32 [Q, k+1, cols], one library call."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         form_workspace_bytes(f, Q, max_query_len, d_queries.numel(), k))
        out = _out(out, (Q, k + 1, f.cols), dev)
        _lib.check(f.fn()(self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len),
                          *_align_args(f, **ask), excl, int(k), out.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out

    # ---- batched, device resident ----
    def _check_queries(self, d_queries, d_q_offsets):
        return _check_queries(self.device, d_queries, d_q_offsets)

    def _prelude(self, d_queries, d_q_offsets, d_exclude_ids, stream, workspace, need):
        """What every batched wrapper does before its one library call: the queries are float64 / int64 on this
        handle's device, the stream is the caller's or the current one, the workspace is the caller's (checked
        against `need` bytes, the wrapper's sizing function for these queries; None leaves the size to the library)
        or a fresh one, the exclusions become a pointer or None.  -> (dev, stream, workspace, exclude pointer)."""
        dev, _ = _check_queries(self.device, d_queries, d_q_offsets)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        need = need or 0
        if workspace is None:
            # per call, from torch's caching allocator (no hipMalloc once warm); pass a persistent
            # one to keep even that off the hot path
            workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
            workspace.record_stream(s)
        elif workspace.device != dev or workspace.dtype != torch.uint8 or workspace.numel() < need:
            raise RuntimeError(f"workspace must be a uint8 tensor of >= {need} bytes on {dev}")
        return dev, s, workspace, d_exclude_ids.data_ptr() if d_exclude_ids is not None else None

    def match(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int,
              min_match: int, cap: int, d_exclude_ids: Optional[torch.Tensor] = None,
              out_hits: Optional[torch.Tensor] = None, out_n: Optional[torch.Tensor] = None,
              stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None,
              algo: int = _lib.ALGO_AUTO):
        """Enqueue Q queries; returns (hits int32[Q,cap,3], hits_n int32[Q]) device tensors.
        `algo`: per-call kernel choice (_lib.ALGO_*); results never depend on it."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         workspace_bytes(Q, max_query_len, total_query_keys=d_queries.numel()))
        out_hits, out_n = _out(out_hits, (Q, cap, 3), dev, "out_hits"), _out(out_n, (Q,), dev, "out_n")
        _lib.check(self.lib.tvz_match(
            self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), int(min_match), excl,
            int(cap), out_hits.data_ptr(), out_n.data_ptr(), ws.data_ptr(), ws.numel(), int(algo), s.cuda_stream))
        return out_hits, out_n

    def match_tol(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, tol: float,
                  min_match: int, cap: int, d_exclude_ids: Optional[torch.Tensor] = None,
                  out_hits: Optional[torch.Tensor] = None, out_n: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None, workspace: Optional[torch.Tensor] = None):
        """The tolerant form of `match` (tvz_match_tol): enqueue Q queries; returns (hits int32[Q,cap,3],
        hits_n int32[Q]) device tensors in match's layout (topk applies)."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         tol_workspace_bytes(Q, max_query_len, d_queries.numel()))
        out_hits, out_n = _out(out_hits, (Q, cap, 3), dev, "out_hits"), _out(out_n, (Q,), dev, "out_n")
        _lib.check(self.lib.tvz_match_tol(
            self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), float(tol), int(min_match),
            excl, int(cap), out_hits.data_ptr(), out_n.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out_hits, out_n

    def match_topk(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int,
                   min_match: int, cap: int, k: int, d_exclude_ids: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                   workspace: Optional[torch.Tensor] = None, algo: int = _lib.ALGO_AUTO) -> torch.Tensor:
        """Sweep + per-shard top-k behind ONE library call (hit lists stay in the workspace):
        -> int32 [Q,k+1,3] = the k best hits by (kth, video_id, count) + a (-1, n_hits, NEVER) row."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         workspace_bytes(Q, max_query_len, cap, k, total_query_keys=d_queries.numel()))
        out = _out(out, (Q, k + 1, 3), dev)
        _lib.check(self.lib.tvz_match_topk(
            self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), int(min_match), excl,
            int(cap), int(k), out.data_ptr(), ws.data_ptr(), ws.numel(), int(algo), s.cuda_stream))
        return out

    def match_tol_topk(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, tol: float,
                       min_match: int, k: int, d_exclude_ids: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                       workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The tolerant sweep with the per-shard top-k kept inside it (tvz_match_tol_topk; min_match 1..5, k <= 64,
        queries of up to 4,095 timestamps): -> int32 [Q,k+1,3] in match_topk's layout.  No cap: the k rows are the
        exact k best and the tail row's n_hits is the true count."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = self._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                         tol_topk_workspace_bytes(Q, max_query_len, d_queries.numel(), k))
        out = _out(out, (Q, k + 1, 3), dev)
        _lib.check(self.lib.tvz_match_tol_topk(
            self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), float(tol), int(min_match),
            excl, int(k), out.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out


class Comm:
    """tvz_comm handle: the RCCL communicator of the sharded match, owned by libtvz.so (a non-Python
    host gets the same path through include/tvz.h).  `unique_id()` on rank 0, ship the 128 bytes to
    the other ranks by any means, then Comm(id, n_ranks, rank, device) on every rank."""

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        _lib.check(_lib.load().tvz_comm_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id: bytes, n_ranks: int, rank: int, device: int = 0):
        self.lib = _lib.load()
        if len(unique_id) != _lib.UNIQUE_ID_BYTES:
            raise RuntimeError("unique id must be 128 bytes")
        h = C.c_void_p()
        _lib.check(self.lib.tvz_comm_init(C.byref(h), C.c_char_p(unique_id), int(n_ranks), int(rank),
                                          int(device)))
        self._h = h
        self.n_ranks, self.rank, self.device = int(n_ranks), int(rank), int(device)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.tvz_comm_destroy(self._h)
            self._h = None

    def info(self) -> Tuple[int, int]:
        """(ranks, rank) as the RCCL communicator inside the library reports them (tvz_comm_info)."""
        n, r = C.c_int32(0), C.c_int32(0)
        _lib.check(self.lib.tvz_comm_info(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def match_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                      max_query_len: int, min_match: int, cap: int, k: int,
                      d_exclude_ids: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None,
                      stream: Optional[torch.cuda.Stream] = None, algo: int = _lib.ALGO_AUTO,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """local match + top-k -> ncclAllGather -> merge, all enqueued on `stream` by ONE library
        call; -> (merged int32 [Q,k,3], totals int32 [Q]), identical on every rank.  `out` =
        (merged, totals) buffers to write into (a caller streaming batches keeps its own)."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = corpus._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                           workspace_bytes(Q, max_query_len, cap, k, self.n_ranks, d_queries.numel()))
        merged, totals = _topk_out(out, Q, k, 3, dev)
        _lib.check(self.lib.tvz_match_sharded(
            corpus._h, self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), int(min_match),
            excl, int(cap), int(k), merged.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws.numel(), int(algo),
            s.cuda_stream))
        return merged, totals

    def match_tol_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                          max_query_len: int, tol: float, min_match: int, k: int,
                          d_exclude_ids: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None,
                          stream: Optional[torch.cuda.Stream] = None,
                          out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """The tolerant form of `match_sharded` (tvz_match_tol_sharded): the sweep that keeps its k best ->
        ncclAllGather -> merge; -> (merged int32 [Q,k,3], totals int32 [Q]: true counts, negative only
        for a query longer than max_query_len)."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = corpus._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                           tol_topk_workspace_bytes(Q, max_query_len, d_queries.numel(), k, self.n_ranks))
        merged, totals = _topk_out(out, Q, k, 3, dev)
        _lib.check(self.lib.tvz_match_tol_sharded(
            corpus._h, self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), float(tol),
            int(min_match), excl, int(k), merged.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws.numel(),
            s.cuda_stream))
        return merged, totals

    def align_topk_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                           max_query_len: int, *, eps: float, max_offset: float, k: int, min_votes: int = 1,
                           min_score: int = 0, d_exclude_ids: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                           out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """tvz_align_topk_sharded: the local alignment top-k -> ncclAllGather of the [Q,k+1,4] blocks -> the merge;
        -> (rows int32 [Q,k,4], totals int32 [Q]), identical on every rank."""
        return self.align_sharded(FORM_BOUNDED, corpus, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, workspace,
                                   stream, out, eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score)

    def align_wide_topk_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                                max_query_len: int, *, eps: float, max_offset: Optional[float] = None, k: int,
                                min_votes: int = 1, min_score: int = 0, contain: bool = False, two_bins: bool = False,
                                d_exclude_ids: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                stream: Optional[torch.cuda.Stream] = None,
                                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """tvz_align_wide_topk_sharded: the local alignment top-k at any shift (`max_offset=None`: the widest) ->
        ncclAllGather of the [Q,k+1,4] blocks -> the wide merge; -> (rows int32 [Q,k,4], totals int32 [Q]), identical
        on every rank."""
        return self.align_sharded(FORM_WIDE, corpus, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, workspace,
                                   stream, out, eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score,
                                   contain=contain, two_bins=two_bins)

    def align_rates_topk_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                                 max_query_len: int, *, eps: float, rates: Sequence[float], max_offset: Optional[float] = None,
                                 k: int, min_votes: int = 1, min_score: int = 0, contain: bool = False, two_bins: bool = False,
                                 d_exclude_ids: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                 stream: Optional[torch.cuda.Stream] = None,
                                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """tvz_align_rates_topk_sharded: the local alignment top-k with rates -> ncclAllGather of the [Q,k+1,5] blocks ->
        its merge; -> (rows int32 [Q,k,5], totals int32 [Q]), identical on every rank."""
        return self.align_sharded(FORM_RATES, corpus, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, workspace,
                                   stream, out, eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score,
                                   rates=rates, contain=contain, two_bins=two_bins)

    def align_span_topk_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                                max_query_len: int, *, eps: float, rates: Sequence[float] = (1.0,),
                                max_offset: Optional[float] = None, k: int, min_votes: int = 1, min_score: int = 0,
                                contain: bool = False, local: bool = False,
                                two_bins: bool = False, d_exclude_ids: Optional[torch.Tensor] = None,
                                workspace: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
        """tvz_align_span_topk_sharded: the local alignment top-k with spans -> ncclAllGather of the [Q,k+1,8] blocks ->
        its merge; -> (rows int32 [Q,k,8], totals int32 [Q]), identical on every rank."""
        return self.align_sharded(FORM_SPAN, corpus, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, workspace,
                                   stream, out, eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score,
                                   rates=rates, contain=contain, local=local, two_bins=two_bins)

    def align_parts_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                            max_query_len: int, d_video_ids: torch.Tensor, *, eps: float, max_offset: Optional[float] = None,
                            rates: Sequence[float] = (1.0,), min_votes: int, max_parts: int,
                            workspace: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_parts_sharded: the local align_parts -> ncclAllGather of the [Q, k, 1 + max_parts, 6] answers -> the
        merge; -> int32 [Q, k, 1 + max_parts, 6], identical on every rank."""
        Q = d_q_offsets.numel() - 1
        ids, id_stride, query_id_stride, k = _parts_ids(d_video_ids, Q, d_queries)
        P = int(max_parts)
        dev, s, ws, _ = corpus._prelude(d_queries, d_q_offsets, None, stream, workspace,
                                        align_parts_sharded_workspace_bytes(Q, max_query_len, d_queries.numel(), k, P,
                                                                            self.n_ranks))
        out = _out(out, (Q, k, 1 + max(P, 0), 6), dev)
        _lib.check(self.lib.tvz_align_parts_sharded(
            corpus._h, self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), ids, id_stride,
            query_id_stride, k, float(eps), _wide_offset(eps, max_offset), *_rates(rates), int(min_votes), P, out.data_ptr(),
            ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out

    def align_candidates_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                                 max_query_len: int, *, c: int, min_count: int = 2, cap: int = 4096,
                                 d_exclude_ids: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                 stream: Optional[torch.cuda.Stream] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_candidates_sharded: the local align_candidates -> ncclAllGather of the [Q, c + 1, 2] blocks -> the
        merge; -> int32 [Q, c + 1, 2], identical on every rank.  Every rank's handle keeps gap codes of one gap_eps."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = corpus._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                           align_candidates_sharded_workspace_bytes(Q, max_query_len, d_queries.numel(), cap,
                                                                                    c, self.n_ranks))
        out = _out(out, (Q, max(int(c), 0) + 1, 2), dev)
        _lib.check(self.lib.tvz_align_candidates_sharded(
            corpus._h, self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), int(min_count), excl,
            int(cap), int(c), out.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out

    def align_candidates_rates_sharded(self, corpus: DeviceCorpus, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                                       max_query_len: int, rates: Sequence[float], *, c: int, min_count: int = 2,
                                       cap: int = 4096, d_exclude_ids: Optional[torch.Tensor] = None,
                                       workspace: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """tvz_align_candidates_rates_sharded: the local align_candidates_rates -> ncclAllGather of the [Q, c + 1, 3]
        blocks -> the merge; -> int32 [Q, c + 1, 3], identical on every rank.  Every rank's handle keeps gap codes of one
        gap_eps, and every rank passes the same `rates`."""
        Q = d_q_offsets.numel() - 1
        h_rates, n_rates = _rates(rates)
        dev, s, ws, excl = corpus._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                           align_candidates_rates_sharded_workspace_bytes(Q, max_query_len, d_queries.numel(),
                                                                                          n_rates, cap, c, self.n_ranks))
        out = _out(out, (Q, max(int(c), 0) + 1, 3), dev)
        _lib.check(self.lib.tvz_align_candidates_rates_sharded(
            corpus._h, self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), h_rates, n_rates,
            int(min_count), excl, int(cap), int(c), out.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream))
        return out

    def align_sharded(self, f: AlignForm, corpus, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, workspace, stream,
                       out, **ask):
        """A form's RCCL call: the prelude with the sharded workspace, the merge's outputs, one library call."""
        Q = d_q_offsets.numel() - 1
        dev, s, ws, excl = corpus._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                           form_workspace_bytes(f, Q, max_query_len, d_queries.numel(), k, self.n_ranks))
        rows, totals = _topk_out(out, Q, k, f.cols, dev)
        _lib.check(f.fn("_sharded")(corpus._h, self._h, d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len),
                                    *_align_args(f, **ask), excl, int(k), rows.data_ptr(), totals.data_ptr(), ws.data_ptr(),
                                    ws.numel(), s.cuda_stream))
        return rows, totals


def _wide_offset(eps: float, max_offset: Optional[float]) -> float:
    """max_offset of the wide calls: None is the widest the library takes, ALIGN_WIDE_MAX_B bins of eps."""
    return ALIGN_WIDE_MAX_B * float(eps) if max_offset is None else float(max_offset)


def _check_queries(device: int, d_queries, d_q_offsets):
    dev = d_queries.device
    if dev.type != "cuda" or dev.index != device:
        raise RuntimeError(f"queries must live on cuda:{device}")
    if d_queries.dtype != torch.float64 or d_q_offsets.dtype != torch.int64:
        raise RuntimeError("queries must be float64 and offsets int64")
    return dev, d_q_offsets.numel() - 1


def _out(out, shape: tuple, dev, name: str = "out"):
    """One int32 output of a batched call: a fresh tensor, or the caller's, checked - the library is told only where
    it starts, and would write past the end of a smaller one."""
    if out is None:
        return torch.empty(shape, dtype=torch.int32, device=dev)
    if out.shape != shape or out.dtype != torch.int32 or out.device != dev or not out.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous int32 {list(shape)} on {dev}")
    return out


def _topk_out(out, Q: int, k: int, width: int, dev):
    """The (rows int32 [Q,k,width], totals int32 [Q]) a merge writes: the caller's `out`, checked, or fresh ones
    (width 3: match hits, 4: alignment rows)."""
    if out is not None:
        rows, totals = out
        if rows.shape != (Q, k, width) or totals.shape != (Q,) or rows.dtype != torch.int32 \
                or totals.dtype != torch.int32 or not rows.is_contiguous():
            raise RuntimeError(f"out must be (int32 [Q,k,{width}], int32 [Q])")
        return rows, totals
    return torch.empty((Q, k, width), dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.int32, device=dev)


def _shards_out(shards, Q: int, k: int, width: int, dev):
    """What the two *_shards calls share: the handle array, the blocks [R,Q,k+1,width] and the merge's outputs."""
    R = len(shards)
    return ((C.c_void_p * R)(*[s._h for s in shards]),
            torch.empty((R, Q, k + 1, width), dtype=torch.int32, device=dev)) + _topk_out(None, Q, k, width, dev)


def topk(lists: torch.Tensor, lists_n: Optional[torch.Tensor], k: int,
         out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Per-query k best hits ordered by (kth, video_id, count).
    lists: int32 [Q,cap,3] or [n_lists,Q,cap,3] (all-gathered shards); -> int32 [Q,k,3]."""
    if lists.dim() == 3:
        lists = lists.unsqueeze(0)
    if lists.dtype != torch.int32 or lists.device.type != "cuda" or not lists.is_contiguous():
        raise RuntimeError("lists must be a contiguous int32 CUDA tensor")
    n_lists, Q, cap, _ = lists.shape
    if out is None:
        out = torch.empty((Q, k, 3), dtype=torch.int32, device=lists.device)
    s = stream if stream is not None else torch.cuda.current_stream(lists.device)
    with torch.cuda.device(lists.device):
        _lib.check(_lib.load().tvz_topk(lists.data_ptr(),
                                        lists_n.data_ptr() if lists_n is not None else None,
                                        n_lists, Q, cap, k, out.data_ptr(), s.cuda_stream))
    return out


def topk_shard(hits: torch.Tensor, hits_n: torch.Tensor, k: int,
               stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Local lists -> int32 [Q,k+1,3]: the k best + a (-1, n_hits, NEVER) totals row."""
    Q, cap, _ = hits.shape
    out = torch.empty((Q, k + 1, 3), dtype=torch.int32, device=hits.device)
    s = stream if stream is not None else torch.cuda.current_stream(hits.device)
    with torch.cuda.device(hits.device):
        _lib.check(_lib.load().tvz_topk_shard(hits.data_ptr(), hits_n.data_ptr(), Q, cap, k,
                                              out.data_ptr(), s.cuda_stream))
    return out


def match_topk_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                      max_query_len: int, min_match: int, cap: int, k: int, workspace: torch.Tensor,
                      d_exclude_ids: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                      algo: int = _lib.ALGO_AUTO):
    """tvz_match_topk on every handle of ONE device + the merge behind one library call:
    -> (blocks int32 [R,Q,k+1,3], merged int32 [Q,k,3], totals int32 [Q])."""
    Q = d_q_offsets.numel() - 1
    dev, s, ws, excl = shards[0]._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace,
                                          workspace_bytes(Q, max_query_len, cap, k, total_query_keys=d_queries.numel()))
    handles, blocks, merged, totals = _shards_out(shards, Q, k, 3, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().tvz_match_topk_shards(
            handles, len(shards), d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len), int(min_match),
            excl, int(cap), int(k), blocks.data_ptr(), merged.data_ptr(), totals.data_ptr(), ws.data_ptr(), ws.numel(),
            int(algo), s.cuda_stream))
    return blocks, merged, totals


def topk_merge(gathered: torch.Tensor, k: int, stream: Optional[torch.cuda.Stream] = None):
    """All-gathered int32 [R,Q,k+1,3] -> (merged int32 [Q,k,3], totals int32 [Q])."""
    R, Q, k1, _ = gathered.shape
    if k1 != k + 1 or not gathered.is_contiguous():
        raise RuntimeError("gathered must be contiguous [R,Q,k+1,3]")
    out = torch.empty((Q, k, 3), dtype=torch.int32, device=gathered.device)
    totals = torch.empty(Q, dtype=torch.int32, device=gathered.device)
    s = stream if stream is not None else torch.cuda.current_stream(gathered.device)
    with torch.cuda.device(gathered.device):
        _lib.check(_lib.load().tvz_topk_merge(gathered.data_ptr(), R, Q, k, out.data_ptr(),
                                              totals.data_ptr(), s.cuda_stream))
    return out, totals


def align_topk_merge(gathered: torch.Tensor, k: int, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                     stream: Optional[torch.cuda.Stream] = None, out=None):
    """tvz_align_topk_merge: the shards' blocks int32 [R,Q,k+1,4] (+ the queries: the order word needs their non-NaN
    counts) -> (rows int32 [Q,k,4], totals int32 [Q]; ALIGN_REFUSED for a query some shard refused)."""
    return form_merge(FORM_BOUNDED, gathered, k, d_queries, d_q_offsets, stream, out)


def align_topk_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                      max_query_len: int, *, eps: float, max_offset: float, k: int, workspace: torch.Tensor,
                      min_votes: int = 1, min_score: int = 0, d_exclude_ids: Optional[torch.Tensor] = None,
                      stream: Optional[torch.cuda.Stream] = None):
    """tvz_align_topk on every handle of ONE device + the merge behind one library call (tvz_align_topk_shards):
    -> (blocks int32 [R,Q,k+1,4], rows int32 [Q,k,4], totals int32 [Q]).  `workspace`: align_topk_workspace_bytes."""
    # (the workspace's size is the library's to judge: it takes one down to a single query's room and refuses the
    # queries that do not fit one by one)
    return form_shards(FORM_BOUNDED, shards, d_queries, d_q_offsets, max_query_len, k, workspace, d_exclude_ids, stream,
                       eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score)


def align_wide_topk_merge(gathered: torch.Tensor, k: int, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                          contain: bool = False, stream: Optional[torch.cuda.Stream] = None, out=None,
                          two_bins: bool = False):
    """tvz_align_wide_topk_merge: align_topk_merge for the blocks of align_wide_topk_block - bins anywhere in
    +-ALIGN_WIDE_MAX_B, every list sorted by align_wide_order_key of the SAME `contain`."""
    return form_merge(FORM_WIDE, gathered, k, d_queries, d_q_offsets, stream, out, contain=contain, two_bins=two_bins)


def align_wide_topk_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                           max_query_len: int, *, eps: float, max_offset: Optional[float] = None, k: int,
                           workspace: torch.Tensor, min_votes: int = 1, min_score: int = 0, contain: bool = False,
                           two_bins: bool = False,
                           d_exclude_ids: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """tvz_align_wide_topk on every handle of ONE device + the wide merge behind one library call
    (tvz_align_wide_topk_shards): -> (blocks int32 [R,Q,k+1,4], rows int32 [Q,k,4], totals int32 [Q]).  `workspace`:
    align_wide_topk_workspace_bytes (its size is the library's to judge, as align_topk_shards')."""
    return form_shards(FORM_WIDE, shards, d_queries, d_q_offsets, max_query_len, k, workspace, d_exclude_ids, stream,
                       eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, contain=contain,
                       two_bins=two_bins)


def align_rates_topk_merge(gathered: torch.Tensor, k: int, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                           contain: bool = False, stream: Optional[torch.cuda.Stream] = None, out=None,
                          two_bins: bool = False):
    """tvz_align_rates_topk_merge: align_wide_topk_merge for the blocks of align_rates_topk_block, int32 [R,Q,k+1,5] ->
    (rows int32 [Q,k,5], totals int32 [Q]); every list sorted by align_rates_order_key of the SAME `contain`, made
    with the same rate list (the rate index is carried, never read)."""
    return form_merge(FORM_RATES, gathered, k, d_queries, d_q_offsets, stream, out, contain=contain, two_bins=two_bins)


def align_rates_topk_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                            max_query_len: int, *, eps: float, rates: Sequence[float], max_offset: Optional[float] = None,
                            k: int, workspace: torch.Tensor, min_votes: int = 1, min_score: int = 0, contain: bool = False,
                            two_bins: bool = False,
                            d_exclude_ids: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """tvz_align_rates_topk on every handle of ONE device + its merge behind one library call
    (tvz_align_rates_topk_shards): -> (blocks int32 [R,Q,k+1,5], rows int32 [Q,k,5], totals int32 [Q]).  `workspace`:
    align_rates_topk_workspace_bytes (its size is the library's to judge, as align_topk_shards')."""
    return form_shards(FORM_RATES, shards, d_queries, d_q_offsets, max_query_len, k, workspace, d_exclude_ids, stream,
                       eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, rates=rates, contain=contain,
                       two_bins=two_bins)


def align_span_topk_merge(gathered: torch.Tensor, k: int, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                          contain: bool = False, local: bool = False, stream: Optional[torch.cuda.Stream] = None, out=None,
                          two_bins: bool = False):
    """tvz_align_span_topk_merge: align_rates_topk_merge for the blocks of align_span_topk_block, int32 [R,Q,k+1,8] ->
    (rows int32 [Q,k,8], totals int32 [Q]); every list sorted by align_span_order_key of the SAME `contain` / `local`.
    With `local` the score is rebuilt from votes, t_last - t_first + 1 and nr; otherwise the span is only carried."""
    return form_merge(FORM_SPAN, gathered, k, d_queries, d_q_offsets, stream, out, contain=contain, local=local,
    two_bins=two_bins)


def align_span_topk_shards(shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                           max_query_len: int, *, eps: float, rates: Sequence[float] = (1.0,),
                           max_offset: Optional[float] = None, k: int, workspace: torch.Tensor, min_votes: int = 1,
                           min_score: int = 0, contain: bool = False, local: bool = False, two_bins: bool = False,
                           d_exclude_ids: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
    """tvz_align_span_topk on every handle of ONE device + its merge behind one library call
    (tvz_align_span_topk_shards): -> (blocks int32 [R,Q,k+1,8], rows int32 [Q,k,8], totals int32 [Q]).  `workspace`:
    align_span_topk_workspace_bytes (its size is the library's to judge, as align_topk_shards')."""
    return form_shards(FORM_SPAN, shards, d_queries, d_q_offsets, max_query_len, k, workspace, d_exclude_ids, stream,
                       eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, rates=rates, contain=contain,
                       local=local, two_bins=two_bins)


def form_merge(f: AlignForm, gathered: torch.Tensor, k: int, d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
               stream: Optional[torch.cuda.Stream] = None, out=None, contain: bool = False, local: bool = False,
               two_bins: bool = False):
    """tvz_<stem>_merge of any form: the blocks int32 [R,Q,k+1,cols] -> (rows int32 [Q,k,cols], totals int32 [Q])."""
    R, Q, k1, w = gathered.shape
    if k1 != k + 1 or w != f.cols or gathered.dtype != torch.int32 or not gathered.is_contiguous():
        raise RuntimeError(f"gathered must be a contiguous int32 [R,Q,k+1,{f.cols}]")
    rows, totals = _topk_out(out, Q, k, f.cols, gathered.device)
    s = stream if stream is not None else torch.cuda.current_stream(gathered.device)
    with torch.cuda.device(gathered.device):
        _lib.check(f.fn("_merge")(gathered.data_ptr(), R, Q, int(k), *_align_flags(f, contain, local, two_bins),
                                  d_queries.data_ptr(),
                                  d_q_offsets.data_ptr(), rows.data_ptr(), totals.data_ptr(), s.cuda_stream))
    return rows, totals


def form_shards(f: AlignForm, shards: Sequence["DeviceCorpus"], d_queries: torch.Tensor, d_q_offsets: torch.Tensor,
                max_query_len: int, k: int, workspace: torch.Tensor, d_exclude_ids: Optional[torch.Tensor] = None,
                stream: Optional[torch.cuda.Stream] = None, **ask):
    """tvz_<stem>_shards of any form: the form's call on every handle of ONE device + its merge behind one library call
    -> (blocks int32 [R,Q,k+1,cols], rows int32 [Q,k,cols], totals int32 [Q]).  `ask`: _align_args' keywords."""
    Q = d_q_offsets.numel() - 1
    dev, s, ws, excl = shards[0]._prelude(d_queries, d_q_offsets, d_exclude_ids, stream, workspace, None)
    handles, blocks, rows, totals = _shards_out(shards, Q, k, f.cols, dev)
    args = _align_args(f, **ask)
    with torch.cuda.device(dev):
        _lib.check(f.fn("_shards")(handles, len(shards), d_queries.data_ptr(), d_q_offsets.data_ptr(), Q, int(max_query_len),
                                   *args, excl, int(k), blocks.data_ptr(), rows.data_ptr(), totals.data_ptr(), ws.data_ptr(),
                                   ws.numel(), s.cuda_stream))
    return blocks, rows, totals


def pack_queries(queries: Sequence[Sequence[float]], device) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Host lists -> (float64 keys, int64 offsets, max_len) on `device`."""
    lens = np.fromiter((len(q) for q in queries), dtype=np.int64, count=len(queries))
    offs = np.zeros(len(queries) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    flat = np.empty(max(int(offs[-1]), 1), dtype=np.float64)
    for q, o, n in zip(queries, offs[:-1], lens):
        if n:
            flat[o:o + n] = np.asarray(q, dtype=np.float64)
    return (torch.from_numpy(flat).to(device), torch.from_numpy(offs).to(device),
            int(lens.max()) if len(queries) else 0)


def align_inputs(queries, exclude_ids, max_query_len: Optional[int], dev):
    """The host-input prelude of every `align_topk`: `queries` as a list of timestamp lists or as device tensors
    (d_queries float64, d_q_offsets int64[Q+1]), `exclude_ids` as None, a list or a device int32 tensor, `max_query_len`
    None for the longest query (at most ALIGN_TOPK_MAX_LEN) -> (d_q, d_off, Q, max_query_len, d_ex) on `dev`."""
    if isinstance(queries, tuple) and len(queries) == 2 and torch.is_tensor(queries[0]):
        d_q, d_off = queries
        _, Q = _check_queries(dev.index, d_q, d_off)
        longest = int((d_off[1:] - d_off[:-1]).max()) if Q and max_query_len is None else 0
    else:
        d_q, d_off, longest = pack_queries(queries, dev)
        Q = len(queries)
    if max_query_len is None:
        max_query_len = min(longest, ALIGN_TOPK_MAX_LEN)
    d_ex = None
    if exclude_ids is not None:
        d_ex = exclude_ids if torch.is_tensor(exclude_ids) else \
            torch.as_tensor(np.asarray(exclude_ids, dtype=np.int32).reshape(-1)).to(dev)
        if d_ex.dtype != torch.int32 or d_ex.numel() != Q or d_ex.device != dev:
            raise RuntimeError(f"exclude_ids must be {Q} int32 values on {dev}")
    return d_q, d_off, Q, max_query_len, d_ex


def thread_workspace(tls: threading.local, need: int, dev) -> torch.Tensor:
    """align_topk's workspace, cached per calling thread in `tls` (calls of several threads overlap); idle again when
    the call's copy to the host has returned."""
    ws = getattr(tls, "align_ws", None)
    if ws is None or ws.numel() < need:
        ws = tls.align_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    return ws
