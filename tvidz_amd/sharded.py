"""Corpus match sharded over the GPUs of one node.

The candidate axis shards naturally: rows are independent.  Each rank (one process per GPU)
holds a contiguous range of the `video_timestamps` rows balanced by key count, queries are
replicated (tiny), every rank runs the local match + per-shard top-k, and ONE all-gather of
[Q, k+1] int32 triples (the extra row carries the shard's hit total) (RCCL over xGMI; <= 768 B per query per rank, latency-bound) is followed by
the same k-way merge on every rank.  There is no other collective on the data path.

The reference has no counterpart (it scans one Postgres table in one Python process,
inspector/db.py:83-91); the merged result is what its find_duplicates + the first-hit rule of
inspector/app.py:235-255 would report, ordered by (kth, video_id).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, corpus as tc
from ._lib import KTH_NEVER


def shard_bounds(offsets: np.ndarray, world: int) -> np.ndarray:
    """Row boundaries [world+1] of contiguous shards with ~equal key counts (not row counts)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    C = offsets.size - 1
    total = int(offsets[-1])
    targets = (np.arange(world + 1, dtype=np.float64) * total / world)
    b = np.searchsorted(offsets, targets, side="left").astype(np.int64)
    b[0], b[-1] = 0, C
    return np.maximum.accumulate(np.clip(b, 0, C))


def shard_csr(ids: np.ndarray, offsets: np.ndarray, keys: np.ndarray, rank: int, world: int):
    b = shard_bounds(offsets, world)
    r0, r1 = int(b[rank]), int(b[rank + 1])
    k0, k1 = int(offsets[r0]), int(offsets[r1])
    return ids[r0:r1], offsets[r0:r1 + 1] - k0, keys[k0:k1]


class HipBackend:
    """The product backend: DeviceCorpus.match + the top-k kernels on this rank's GPU."""

    supports_tolerance = True

    def __init__(self, corpus):
        self.corpus = corpus

    def match(self, d_q, d_off, max_len, min_match, cap, d_excl):
        return self.corpus.match(d_q, d_off, max_len, min_match, cap, d_exclude_ids=d_excl)

    def local_topk(self, d_q, d_off, max_len, min_match, cap, k, d_excl, tolerance: float = 0.0):
        """sweep + per-shard top-k behind one library call (tvz_match_topk; with a tolerance tvz_match_tol_topk,
        the sweep that keeps its k best itself and has no cap)."""
        if tolerance:
            return self.corpus.match_tol_topk(d_q, d_off, max_len, tolerance, min_match, k, d_exclude_ids=d_excl)
        return self.corpus.match_topk(d_q, d_off, max_len, min_match, cap, k, d_exclude_ids=d_excl)

    def topk_shard(self, hits, hits_n, k):
        return tc.topk_shard(hits, hits_n, k)

    def topk_merge(self, gathered, k):
        return tc.topk_merge(gathered, k)

    align_forms = tc.ALIGN_FORMS        # the forms of the alignment top-k this backend answers: all four

    def local_align(self, form, d_q, d_off, max_len, k, d_excl, **ask):
        """this rank's alignment top-k block of `form` (tvz_<stem>): int32 [Q, k+1, form.cols] on the device"""
        return self.corpus._align_block(form, d_q, d_off, max_len, k, d_excl, None, None, None, **ask)

    def align_merge(self, form, gathered, k, d_q, d_off, **flags):
        return tc.form_merge(form, gathered, k, d_q, d_off, **flags)

    def local_parts(self, d_q, d_off, max_len, d_ids, **ask):
        """this rank's answer to a parts call (tvz_align_parts): int32 [Q, k, 1 + max_parts, 6] on the device"""
        return self.corpus.align_parts_block(d_q, d_off, max_len, d_ids, **ask)

    def parts_merge(self, gathered):
        return tc.align_parts_merge_device(gathered)

    def local_candidates(self, d_q, d_off, max_len, **ask):
        """this rank's candidate ids (tvz_align_candidates; `ask`: c, min_count, cap, d_exclude_ids): the block int32
        [Q, c + 1, 2] on the device"""
        return self.corpus.align_candidates_block(d_q, d_off, max_len, **ask)

    def candidates_merge(self, gathered):
        return tc.align_candidates_merge_device(gathered)

    def local_candidates_rates(self, d_q, d_off, max_len, rates, **ask):
        """this rank's candidate ids at a list of rates (tvz_align_candidates_rates; `ask`: c, min_count, cap,
        d_exclude_ids): the block int32 [Q, c + 1, 3] on the device"""
        return self.corpus.align_candidates_rates_block(d_q, d_off, max_len, rates, **ask)

    def candidates_rates_merge(self, gathered):
        return tc.align_candidates_rates_merge_device(gathered)


def _two_bins(two_bins: bool) -> dict:
    return {"two_bins": True} if two_bins else {}


class _AlignForwards:
    """The near-duplicate search as both matchers offer it on top of their `align(form, ...)` and `align_forms`: the
    public calls are forwards that name their form, the supports_* flags views of `align_forms`.  `two_bins`
    (TVZ_ALIGN_TWO_BINS) is handed on only where it is set: a backend that has never heard of it keeps working."""

    def align_topk(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                   max_offset: float, k: int, min_votes: int = 1, min_score: int = 0,
                   d_exclude_ids: Optional[torch.Tensor] = None):
        """`align` for tvz_align_topk: -> (rows int32 [Q,k,4], totals int32 [Q])."""
        return self.align(tc.FORM_BOUNDED, d_queries, d_q_offsets, max_query_len, k=k, d_exclude_ids=d_exclude_ids,
                          eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score)

    def align_wide_topk(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                        max_offset: Optional[float] = None, k: int, min_votes: int = 1, min_score: int = 0,
                        contain: bool = False, d_exclude_ids: Optional[torch.Tensor] = None, two_bins: bool = False):
        """`align` for tvz_align_wide_topk: align_topk at any shift (`max_offset=None`: the widest), scored by the
        containment with `contain`."""
        return self.align(tc.FORM_WIDE, d_queries, d_q_offsets, max_query_len, k=k, d_exclude_ids=d_exclude_ids,
                          eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, contain=contain,
                          **_two_bins(two_bins))

    def align_rates_topk(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                         rates, max_offset: Optional[float] = None, k: int, min_votes: int = 1, min_score: int = 0,
                         contain: bool = False, d_exclude_ids: Optional[torch.Tensor] = None, two_bins: bool = False):
        """`align` for tvz_align_rates_topk: align_wide_topk for copies played at another speed -> (rows int32 [Q,k,5],
        totals int32 [Q])."""
        return self.align(tc.FORM_RATES, d_queries, d_q_offsets, max_query_len, k=k, d_exclude_ids=d_exclude_ids,
                          eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, rates=tuple(rates),
                          contain=contain, **_two_bins(two_bins))

    def align_span_topk(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, eps: float,
                        rates=(1.0,), max_offset: Optional[float] = None, k: int, min_votes: int = 1, min_score: int = 0,
                        contain: bool = False, local: bool = False, d_exclude_ids: Optional[torch.Tensor] = None,
                        two_bins: bool = False):
        """`align` for tvz_align_span_topk: align_rates_topk with every hit's span, scored inside it with `local` ->
        (rows int32 [Q,k,8], totals int32 [Q])."""
        return self.align(tc.FORM_SPAN, d_queries, d_q_offsets, max_query_len, k=k, d_exclude_ids=d_exclude_ids,
                          eps=eps, max_offset=max_offset, min_votes=min_votes, min_score=min_score, rates=tuple(rates),
                          contain=contain, local=local, **_two_bins(two_bins))

    @property
    def supports_align_topk(self) -> bool:
        return tc.FORM_BOUNDED in self.align_forms

    @property
    def supports_align_rates(self) -> bool:
        return tc.FORM_RATES in self.align_forms

    @property
    def supports_align_span(self) -> bool:
        return tc.FORM_SPAN in self.align_forms

    @property
    def supports_align_wide(self) -> bool:
        return tc.FORM_WIDE in self.align_forms


class ShardedMatcher(_AlignForwards):
    """rank-local shard + ONE all-gather of per-shard top-k (+ hit totals) + identical merge on
    every rank."""

    def __init__(self, backend, k: int = 64, cap: int = 1024, group=None,
                 always_collective: bool = False):
        self.backend = backend
        self.k = int(k)
        self.cap = max(int(cap), self.k)
        self.group = group
        inited = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if inited else 1
        self.rank = dist.get_rank(group) if inited else 0
        # run the all-gather even in a 1-rank group (used to rehearse the RCCL path on one GPU)
        self.collective = self.world > 1 or (always_collective and inited)

    @property
    def supports_tolerance(self) -> bool:
        return bool(getattr(self.backend, "supports_tolerance", False))

    def submit(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int,
               min_match: int, d_exclude_ids: Optional[torch.Tensor] = None, tolerance: float = 0.0):
        """Enqueue local match + per-shard top-k and START the all-gather; returns a ticket for
        finish().  Submitting batch i+1 before finishing batch i overlaps the collective of one
        batch with the match kernels of the next (RCCL runs on its own stream).
        `tolerance` > 0: the opt-in tolerant match; the backend must say `supports_tolerance`."""
        if tolerance:
            if not self.supports_tolerance:
                raise RuntimeError(f"{type(self.backend).__name__} has no tolerant match (supports_tolerance)")
            local = self.backend.local_topk(d_queries, d_q_offsets, max_query_len, min_match, self.cap,
                                            self.k, d_exclude_ids, tolerance=float(tolerance))
        elif hasattr(self.backend, "local_topk"):
            local = self.backend.local_topk(d_queries, d_q_offsets, max_query_len, min_match, self.cap,
                                            self.k, d_exclude_ids)     # [Q, k+1, 3]
        else:
            hits, n = self.backend.match(d_queries, d_q_offsets, max_query_len, min_match, self.cap,
                                         d_exclude_ids)
            local = self.backend.topk_shard(hits, n, self.k)          # [Q, k+1, 3]
        return self._all_gather_blocks(local, async_op=True) + (local,)

    def _all_gather_blocks(self, local: torch.Tensor, async_op: bool):
        """This rank's block [Q, k+1, w] -> (every rank's, as [world, Q, k+1, w]; the collective's work handle, None
        where there was none to start or to wait for)."""
        if not self.collective:
            return local.view((1,) + tuple(local.shape)), None
        # dim-0 concatenation is the layout both RCCL and gloo accept for all_gather_into_tensor
        flat = torch.empty((self.world * local.shape[0],) + tuple(local.shape[1:]), dtype=torch.int32,
                           device=local.device)
        work = dist.all_gather_into_tensor(flat, local.contiguous(), group=self.group, async_op=async_op)
        return flat.view((self.world,) + tuple(local.shape)), work

    def finish(self, ticket):
        """-> (merged int32 [Q,k,3] of (video_id, count, kth), total_hits int32 [Q]) — identical on
        every rank.  total_hits > k means the list was truncated to the k best; a NEGATIVE total
        means a shard's hit list overflowed `cap` (re-run that query with a larger cap)."""
        gathered, work, _keepalive = ticket
        if work is not None:
            work.wait()                     # makes the current stream wait for the collective
        return self.backend.topk_merge(gathered, self.k)

    def match_topk(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int,
                   min_match: int, d_exclude_ids: Optional[torch.Tensor] = None, tolerance: float = 0.0):
        return self.finish(self.submit(d_queries, d_q_offsets, max_query_len, min_match, d_exclude_ids,
                                       tolerance=tolerance))

    @property
    def align_forms(self) -> tuple:
        """The forms of the alignment top-k (corpus.ALIGN_FORMS) `align` answers: the backend's."""
        return tuple(getattr(self.backend, "align_forms", ()))

    def align(self, form, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, k: int,
              d_exclude_ids: Optional[torch.Tensor] = None, **ask):
        """The near-duplicate search over the sharded table, for `form` and what the call may `ask` of it (eps,
        max_offset, min_votes, min_score, its flags): the local block [Q, k+1, form.cols] -> ONE all-gather -> the merge
        by the contract's order and the ask's score kind, identical on every rank: -> (rows int32 [Q,k,form.cols],
        totals int32 [Q]; corpus.ALIGN_REFUSED for a query some rank refused).  `k` is the call's own, not the
        matcher's."""
        if form not in self.align_forms:
            raise RuntimeError(f"{type(self.backend).__name__} has no {form.stem}")
        local = self.backend.local_align(form, d_queries, d_q_offsets, max_query_len, int(k), d_exclude_ids, **ask)
        gathered, _ = self._all_gather_blocks(local, async_op=False)
        return self.backend.align_merge(form, gathered, k, d_queries, d_q_offsets, **{n: ask[n] for n in form.flags})

    @property
    def supports_align_parts(self) -> bool:
        """Does `parts` answer?  Only over a backend with the local call and the merge."""
        return hasattr(self.backend, "local_parts") and hasattr(self.backend, "parts_merge")

    def parts(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, d_video_ids: torch.Tensor,
              **ask):
        """Every aligned part of named stored videos over the sharded table (tvz_align_parts; `ask`: eps, max_offset,
        rates, min_votes, max_parts): this rank's answer [Q, k, 1 + max_parts, 6] -> ONE all-gather -> the merge that
        keeps, per pair, the answer with the most part-0 votes among the ranks that hold a row of the id (the lower
        rank on a tie), sums n_rows and keeps a refusal: identical on every rank."""
        if not self.supports_align_parts:
            raise RuntimeError(f"{type(self.backend).__name__} has no align_parts")
        local = self.backend.local_parts(d_queries, d_q_offsets, max_query_len, d_video_ids, **ask)
        gathered, _ = self._all_gather_blocks(local, async_op=False)
        return self.backend.parts_merge(gathered)

    @property
    def supports_align_candidates(self) -> bool:
        """Does `candidates` answer?  Only over a backend with the local call and the merge."""
        return hasattr(self.backend, "local_candidates") and hasattr(self.backend, "candidates_merge")

    def candidates(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, c: int,
                   min_count: int = 2, cap: int = 4096, d_exclude_ids: Optional[torch.Tensor] = None):
        """The candidate ids from the gap codes over the sharded table (tvz_align_candidates; every rank's shard keeps
        codes of the same gap_eps): this rank's block [Q, c + 1, 2] -> ONE all-gather -> the merge that keeps the c
        best of all ranks' rows and sums their totals (include/tvz_gap_shards.h), identical on every rank: -> the
        block int32 [Q, c + 1, 2].  More than 16 ranks are merged in groups of 16, the groups' answers again."""
        if not self.supports_align_candidates:
            raise RuntimeError(f"{type(self.backend).__name__} has no align_candidates")
        local = self.backend.local_candidates(d_queries, d_q_offsets, max_query_len, c=int(c), min_count=int(min_count),
                                              cap=int(cap), d_exclude_ids=d_exclude_ids)
        gathered, _ = self._all_gather_blocks(local, async_op=False)
        return merge_candidate_blocks(self.backend.candidates_merge, gathered)

    @property
    def supports_align_candidate_rates(self) -> bool:
        """Does `candidates_rates` answer?  Only over a backend with the local call and the merge."""
        return hasattr(self.backend, "local_candidates_rates") and hasattr(self.backend, "candidates_rates_merge")

    def candidates_rates(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, rates, *, c: int,
                         min_count: int = 2, cap: int = 4096, d_exclude_ids: Optional[torch.Tensor] = None):
        """`candidates` for copies played at another speed (tvz_align_candidates_rates with `rates`, the same on every
        rank): this rank's block [Q, c + 1, 3] -> ONE all-gather -> the merge that keeps one row per id - its largest
        best at the smallest rate index -, the c best of them, and sums the totals (include/tvz_gap_rates_shards.h),
        identical on every rank: -> the block int32 [Q, c + 1, 3].  More than 16 ranks are merged in groups of 16."""
        if not self.supports_align_candidate_rates:
            raise RuntimeError(f"{type(self.backend).__name__} has no align_candidates_rates")
        local = self.backend.local_candidates_rates(d_queries, d_q_offsets, max_query_len, tuple(rates), c=int(c),
                                                    min_count=int(min_count), cap=int(cap), d_exclude_ids=d_exclude_ids)
        gathered, _ = self._all_gather_blocks(local, async_op=False)
        return merge_candidate_blocks(self.backend.candidates_rates_merge, gathered)


def merge_candidate_blocks(merge, gathered):
    """`merge` (up to corpus.ALIGN_CANDIDATES_MERGE_MAX_LISTS blocks -> one; the plain or the rates merge, which take
    as many) over any number of them [R, Q, c + 1, 2 or 3]: groups of up to 16, then the groups' answers, until one is
    left - both rules are associative."""
    n = tc.ALIGN_CANDIDATES_MERGE_MAX_LISTS
    while gathered.shape[0] > n:
        lib = torch if torch.is_tensor(gathered) else np
        gathered = lib.stack([merge(gathered[i:i + n]) for i in range(0, gathered.shape[0], n)])
    return merge(gathered)


def make_comm(device: int, group=None):
    """Create the libtvz RCCL communicator of this rank.  torch.distributed (any backend) is used
    ONLY to ship rank 0's 128-byte unique id; a non-Python host ships it by its own means."""
    if not dist.is_initialized():          # a single process: a one-rank communicator, same data path
        return tc.Comm(tc.Comm.unique_id(), 1, 0, device)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    box = [tc.Comm.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0,
                               group=group)
    return tc.Comm(box[0], world, rank, device)


class _Slot:
    """What one of RcclShardedMatcher's side streams owns: its event, submit's workspace and (merged, totals), and
    align's own pair (its rows are the form's width and `k` is the call's own)."""
    __slots__ = ("stream", "event", "ws", "out", "near_ws", "near_out", "parts_out", "cand_out", "cand_rates_out")

    def __init__(self, stream):
        self.stream, self.event = stream, torch.cuda.Event()
        self.ws = self.out = self.near_ws = self.near_out = self.parts_out = self.cand_out = self.cand_rates_out = None


class RcclShardedMatcher(_AlignForwards):
    """The sharded match with the collective BEHIND the C ABI (tvz_match_sharded): local sweep +
    per-shard top-k -> ncclAllGather -> merge are enqueued on one HIP stream by one library call.
    submit() alternates between two side streams with their own workspaces, so the all-gather and
    merge of batch i overlap the sweep of batch i+1; finish() makes the current stream wait for
    the ticket.  Same results as ShardedMatcher (which keeps the merge logic testable on gloo)."""

    def __init__(self, corpus, comm, k: int = 64, cap: int = 1024, n_streams: int = 2, priority: int = 0,
                 algo: int = 0):
        """`priority=-1`: the service's ticks - a few tiny launches that should not queue behind the upload
        workers' scene kernels."""
        self.corpus, self.comm = corpus, comm
        self.algo = int(algo)               # _lib.ALGO_* (+ ALGO_PAIR / ALGO_NO_PAIR) of every batch
        if not self.algo & (_lib.ALGO_PAIR | _lib.ALGO_NO_PAIR) and n_streams < 3:
            # two queries per lookup block pay off when a THIRD batch's blocks fill the longer tail of a launch
            # (42 against 46 us per batch on a 1/8 shard); with two batches in flight they cost (57 against 52)
            self.algo |= _lib.ALGO_NO_PAIR
        if not self.algo & (_lib.ALGO_WAVE | _lib.ALGO_NO_WAVE | _lib.ALGO_PAIR):
            # a stream of batches: on a shard of one sub-index the lookup that gives every query to one wave executes
            # a third fewer instructions per batch than the block kernel (which answers a LONE batch sooner: tvz.h)
            self.algo |= _lib.ALGO_PREFER_WAVE
        self.k = int(k)
        self.cap = max(int(cap), self.k)
        self.world, self.rank = comm.n_ranks, comm.rank
        self.collective = True
        self.dev = torch.device("cuda", corpus.device)
        self._slots = [_Slot(torch.cuda.Stream(self.dev, priority=priority)) for _ in range(n_streams)]
        self._i = 0
        self._plans = {}                    # (slot, query tensors, shape) -> the library call's arguments (submit)
        self._lib = _lib
        self._call = comm.lib.tvz_match_sharded
        self._call_tol = comm.lib.tvz_match_tol_sharded

    supports_tolerance = True

    def _next_slot(self) -> _Slot:
        """The side stream a call runs on; the calls take them in turn."""
        slot = self._slots[self._i]
        self._i = (self._i + 1) % len(self._slots)
        return slot

    def _drop_plans(self, i: int) -> None:
        self._plans = {k_: v for k_, v in self._plans.items() if k_[0] != i}

    def submit(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int,
               min_match: int, d_exclude_ids: Optional[torch.Tensor] = None, inputs_ready: bool = False,
               tolerance: float = 0.0):
        """Enqueue one batch; the returned ticket's tensors belong to this matcher and are
        overwritten by the submit() `n_streams` calls later - consume them (or copy) before that.
        Nothing is allocated per batch: at 8 GPUs a batch is ~0.1 ms of device time, and fresh
        output tensors + events per call were a comparable amount of host time.
        `inputs_ready`: the query tensors are complete already and nothing pending on the caller's
        stream still reads this slot's previous results, so the side stream does not wait for the
        caller's stream.  That wait
        is a marker in the caller's queue BEHIND the caller's earlier finish() waits - a chain of
        cross-queue barriers the command processor resolves in 10-40 us, which at 8 GPUs (a batch
        is ~60 us of kernels) left the chip idle between two batches' match kernels
        (profiles/r3_shard_pipeline.txt).
        `tolerance` > 0: the opt-in tolerant match (tvz_match_tol_sharded: the sweep keeps its k best itself, `cap`
        and `algo` play no part); it is part of the plan's key and the plan has its own workspace size."""
        tolerance = float(tolerance)
        i = self._i                         # (the rotation stays written out here: submit is the hot path)
        self._i = (i + 1) % len(self._slots)
        slot = self._slots[i]
        st = slot.stream
        # Steady state: the same query tensors come round again (a service's staging slots, a benchmark's rotating
        # batches).  Everything that does not change with them - workspace, outputs, the seventeen arguments of the
        # library call - is kept as a PLAN per (slot, tensors, shape): a batch on a 1/8 shard is ~40 us of GPU time and
        # the un-planned submit was 30 us of interpreter time, the pipeline's actual bound.
        key = (i, d_queries.data_ptr(), d_q_offsets.data_ptr(), int(max_query_len), int(min_match),
               d_exclude_ids.data_ptr() if d_exclude_ids is not None else 0, d_queries.numel(), d_q_offsets.numel())
        if tolerance:
            key += (tolerance,)
        plan = self._plans.get(key)
        if plan is None:
            _, Q = self.corpus._check_queries(d_queries, d_q_offsets)
            if tolerance:
                need = tc.tol_topk_workspace_bytes(Q, max_query_len, d_queries.numel(), self.k, self.world)
            else:
                need = tc.workspace_bytes(Q, max_query_len, self.cap, self.k, self.world, d_queries.numel())
            if slot.ws is None or slot.ws.numel() < need:
                slot.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
                self._drop_plans(i)         # (their workspace is gone)
            if slot.out is None or slot.out[0].shape[0] != Q:
                slot.out = tc._topk_out(None, Q, self.k, 3, self.dev)
                self._drop_plans(i)
            merged, totals = slot.out
            head = (self.corpus._h, self.comm._h, key[1], key[2], Q, key[3])
            tail = (self.k, merged.data_ptr(), totals.data_ptr(), slot.ws.data_ptr(), slot.ws.numel())
            if tolerance:
                call = self._call_tol
                args = head + (tolerance, key[4], key[5] or None) + tail + (st.cuda_stream,)
            else:
                call = self._call
                args = head + (key[4], key[5] or None, self.cap) + tail + (self.algo, st.cuda_stream)
            if len(self._plans) > 256:
                self._plans.clear()
            plan = self._plans[key] = (args, merged, totals, slot.ws, call)
        args, merged, totals, _ws, call = plan
        if not inputs_ready:
            st.wait_stream(torch.cuda.current_stream(self.dev))   # the queries are complete before the match reads them
        rc = call(*args)
        if rc:
            self._lib.check(rc)
        ev = slot.event
        ev.record(st)
        return (merged, totals, ev)

    def finish(self, ticket, host: bool = False):
        """Order the consumer behind the batch: the caller's current stream waits for it (default),
        or - `host=True`, what a consumer that reads the verdicts on the host does anyway - the
        calling thread does (no barrier packet in the caller's queue)."""
        merged, totals, ev = ticket
        if host:
            ev.synchronize()
        else:
            torch.cuda.current_stream(self.dev).wait_event(ev)
        return merged, totals

    def match_topk(self, d_queries, d_q_offsets, max_query_len, min_match, d_exclude_ids=None, tolerance: float = 0.0):
        return self.finish(self.submit(d_queries, d_q_offsets, max_query_len, min_match, d_exclude_ids,
                                       tolerance=tolerance))

    align_forms = tuple(f for f in tc.ALIGN_FORMS if f.rccl)

    def align(self, form, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, k: int,
              d_exclude_ids: Optional[torch.Tensor] = None, **ask):
        """The near-duplicate search over the sharded table behind ONE library call (tvz_<stem>_sharded), for `form`
        and what the call may `ask` of it, as ShardedMatcher.align: the local alignment top-k -> ncclAllGather of the
        [Q, k+1, form.cols] blocks -> the merge, on the next of the matcher's side streams; the current stream waits
        for it.  -> (rows int32 [Q,k,form.cols], totals int32 [Q]), this matcher's tensors, overwritten `n_streams`
        calls later.  Its own workspace (`k` is the call's own) and no plan: the near-duplicate report is one call per
        upload, not the tick's stream of batches."""
        if form not in self.align_forms:
            raise RuntimeError(f"{type(self).__name__} has no {form.stem}: the library has no tvz_{form.stem}_sharded")
        return self._near_call(form, d_queries, d_q_offsets, max_query_len, int(k), d_exclude_ids, **ask)

    def _near_call(self, form, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids, **ask):
        """`align` on the next side stream: its near workspace and (rows, totals), the form's one library call, the
        current stream's wait for it."""
        slot = self._next_slot()
        st = slot.stream
        _, Q = self.corpus._check_queries(d_queries, d_q_offsets)
        need = tc.form_workspace_bytes(form, Q, max_query_len, d_queries.numel(), k, self.world)
        if slot.near_ws is None or slot.near_ws.numel() < need:
            slot.near_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.dev)
        if slot.near_out is None or slot.near_out[0].shape != (Q, k, form.cols):
            slot.near_out = tc._topk_out(None, Q, k, form.cols, self.dev)
        st.wait_stream(torch.cuda.current_stream(self.dev))       # the queries are complete; the slot's last answer is read
        rows, totals = self.comm.align_sharded(form, self.corpus, d_queries, d_q_offsets, max_query_len, k, d_exclude_ids,
                                               slot.near_ws, st, slot.near_out, **ask)
        slot.event.record(st)
        torch.cuda.current_stream(self.dev).wait_event(slot.event)
        return rows, totals


    supports_align_parts = "tvz_align_parts_sharded" in _lib.SIGNATURES

    def parts(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, d_video_ids: torch.Tensor,
              **ask):
        """ShardedMatcher.parts behind ONE library call (tvz_align_parts_sharded): the local tvz_align_parts ->
        ncclAllGather of the [Q, k, 1 + max_parts, 6] answers -> the merge, on the next of the matcher's side streams
        with the slot's near workspace; the current stream waits for it.  -> int32 [Q, k, 1 + max_parts, 6], this
        matcher's tensor, overwritten `n_streams` calls later."""
        if not self.supports_align_parts:
            raise RuntimeError(f"{type(self).__name__} has no align_parts: the library has no tvz_align_parts_sharded")
        slot = self._next_slot()
        st = slot.stream
        _, Q = self.corpus._check_queries(d_queries, d_q_offsets)
        k, P = int(d_video_ids.shape[1]), int(ask["max_parts"])
        need = tc.align_parts_sharded_workspace_bytes(Q, max_query_len, d_queries.numel(), k, P, self.world)
        if slot.near_ws is None or slot.near_ws.numel() < need:
            slot.near_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.dev)
        if slot.parts_out is None or slot.parts_out.shape != (Q, k, 1 + P, 6):
            slot.parts_out = torch.empty((Q, k, 1 + max(P, 0), 6), dtype=torch.int32, device=self.dev)
        st.wait_stream(torch.cuda.current_stream(self.dev))       # the queries and ids are complete; the slot's last answer is read
        out = self.comm.align_parts_sharded(self.corpus, d_queries, d_q_offsets, max_query_len, d_video_ids,
                                            workspace=slot.near_ws, stream=st, out=slot.parts_out, **ask)
        slot.event.record(st)
        torch.cuda.current_stream(self.dev).wait_event(slot.event)
        return out

    supports_align_candidates = "tvz_align_candidates_sharded" in _lib.GAP_SHARD_SIGNATURES

    def candidates(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, *, c: int,
                   min_count: int = 2, cap: int = 4096, d_exclude_ids: Optional[torch.Tensor] = None):
        """ShardedMatcher.candidates behind ONE library call (tvz_align_candidates_sharded): the local
        tvz_align_candidates -> ncclAllGather of the [Q, c + 1, 2] blocks -> the merge, on the next of the matcher's side
        streams with the slot's near workspace; the current stream waits for it.  -> int32 [Q, c + 1, 2], this
        matcher's tensor, overwritten `n_streams` calls later."""
        slot = self._next_slot()
        st = slot.stream
        _, Q = self.corpus._check_queries(d_queries, d_q_offsets)
        c = int(c)
        need = tc.align_candidates_sharded_workspace_bytes(Q, max_query_len, d_queries.numel(), cap, c, self.world)
        if slot.near_ws is None or slot.near_ws.numel() < need:
            slot.near_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.dev)
        if slot.cand_out is None or slot.cand_out.shape != (Q, c + 1, 2):
            slot.cand_out = torch.empty((Q, max(c, 0) + 1, 2), dtype=torch.int32, device=self.dev)
        st.wait_stream(torch.cuda.current_stream(self.dev))       # the queries are complete; the slot's last answer is read
        out = self.comm.align_candidates_sharded(self.corpus, d_queries, d_q_offsets, max_query_len, c=c, min_count=min_count,
                                                 cap=cap, d_exclude_ids=d_exclude_ids, workspace=slot.near_ws, stream=st,
                                                 out=slot.cand_out)
        slot.event.record(st)
        torch.cuda.current_stream(self.dev).wait_event(slot.event)
        return out

    supports_align_candidate_rates = "tvz_align_candidates_rates_sharded" in _lib.GAP_RATE_SHARD_SIGNATURES

    def candidates_rates(self, d_queries: torch.Tensor, d_q_offsets: torch.Tensor, max_query_len: int, rates, *, c: int,
                         min_count: int = 2, cap: int = 4096, d_exclude_ids: Optional[torch.Tensor] = None):
        """ShardedMatcher.candidates_rates behind ONE library call (tvz_align_candidates_rates_sharded): the local
        tvz_align_candidates_rates -> ncclAllGather of the [Q, c + 1, 3] blocks -> the merge, on the next of the
        matcher's side streams with the slot's near workspace; the current stream waits for it.  -> int32 [Q, c + 1, 3],
        this matcher's tensor, overwritten `n_streams` calls later."""
        slot = self._next_slot()
        st = slot.stream
        _, Q = self.corpus._check_queries(d_queries, d_q_offsets)
        c, rates = int(c), tuple(rates)
        need = tc.align_candidates_rates_sharded_workspace_bytes(Q, max_query_len, d_queries.numel(), len(rates), cap, c,
                                                                 self.world)
        if slot.near_ws is None or slot.near_ws.numel() < need:
            slot.near_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.dev)
        if slot.cand_rates_out is None or slot.cand_rates_out.shape != (Q, c + 1, 3):
            slot.cand_rates_out = torch.empty((Q, max(c, 0) + 1, 3), dtype=torch.int32, device=self.dev)
        st.wait_stream(torch.cuda.current_stream(self.dev))       # the queries are complete; the slot's last answer is read
        out = self.comm.align_candidates_rates_sharded(self.corpus, d_queries, d_q_offsets, max_query_len, rates, c=c,
                                                       min_count=min_count, cap=cap, d_exclude_ids=d_exclude_ids,
                                                       workspace=slot.near_ws, stream=st, out=slot.cand_rates_out)
        slot.event.record(st)
        torch.cuda.current_stream(self.dev).wait_event(slot.event)
        return out


def verdicts_from_topk(merged: np.ndarray):
    """Per query: (k*, sorted dup ids) = rows whose kth is minimal (app.py:235-255 batch form),
    or (None, []) when nothing reached min_match.  `truncated` is True when the tie set may
    exceed k (caller should re-query with a larger k)."""
    out = []
    for rows in merged:
        valid = rows[rows[:, 0] >= 0]
        valid = valid[valid[:, 2] < KTH_NEVER]
        if valid.shape[0] == 0:
            out.append((None, [], False))
            continue
        kstar = int(valid[:, 2].min())
        ids = sorted(int(v) for v in valid[valid[:, 2] == kstar][:, 0])
        truncated = bool(rows[-1, 0] >= 0 and rows[-1, 2] == kstar)
        out.append((kstar, ids, truncated))
    return out
