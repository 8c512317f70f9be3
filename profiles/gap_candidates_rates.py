#!/usr/bin/env python3
"""Candidate ids at a list of rates against the rates sweep, on the table of profiles/gap_candidates.py (100k rows x ~200
cuts, synth_timestamp_corpus; eps 1/30, gap_eps 1/30).  Queries: stored rows of 200 cuts played at 25/24 and shifted,
x = (stored - 3600) / (25/24).
   cand R      tvz_align_candidates_rates at n_rates = 1, 3 and 8, C = 16
   cand+parts  ... followed by tvz_align_parts over the block's ids with the same rate list, max_parts = 1
   sweep R     tvz_align_span_topk with TVZ_ALIGN_LOCAL and the same rate list, k = 16: the sweep it replaces
each at Q = 1, 16, 64 in ONE process on one GPU; device events around the enqueued calls, medians with IQR.  Also per
line: the share of queries whose true row is the block's first, and the (row, rate) pairs per query (n_pairs).
In front of that table, like for like: tvz_align_candidates against the new call with the rate list (1.0,) on the SAME
queries (the stored rows shifted by an hour, which rate 1 finds), the two timed in turns A B A B; the blocks are compared.
   timeout -k 10 1100 python3 profiles/gap_candidates_rates.py > gap_candidates_rates.txt"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--sweep-reps", type=int, default=3)
ap.add_argument("--turns-only", action="store_true", help="the A B A B table only (a parent build against a branch build)")
args = ap.parse_args()

import torch  # noqa: E402

from tvidz_amd import corpus as tc, synth  # noqa: E402

dev = torch.device("cuda:0")
EPS, GAP_EPS, K, C, NQ, SHIFT, MIN_VOTES, SPEED = 1.0 / 30, 1.0 / 30, 16, 16, 200, 3600.0, 8, 25 / 24
RATE_LISTS = ((SPEED,), (1.0, 24 / 25, SPEED), (1.0, 24 / 25, SPEED, 1000 / 1001, 1001 / 1000, 1.25, 0.8, 1.1))
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()          # rows with at least NQ cuts
queries = [((keys[offs[r]:offs[r + 1]][:NQ] - SHIFT) / SPEED).tolist() for r in src]
print(f"gap candidates at a list of rates: {args.rows} rows, {int(offs[-1])} keys, queries of {NQ} cuts played at 25/24 and moved "
      f"by {SHIFT:g} s, eps {EPS:.4f}, gap_eps {GAP_EPS:.4f}, C = K = {C}, {torch.cuda.get_device_name(0)}")


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return f"{med:9.4f} ({q3 - q1:.4f})"


def timed(fn, reps):
    fn()                                                                          # warm-up
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
dc.set_gap_index(GAP_EPS)
torch.cuda.synchronize()
print("gap_index_stats:", dc.gap_index_stats())
print()
print("the plain call against the new call at the rate list (1.0,), the same shifted queries, in turns; ms per call, median (IQR)")
for Q in (1, 16, 64):
    qs = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src[:Q]]
    d_q, d_off, L = tc.pack_queries(qs, dev)
    ws_0 = torch.empty(tc.align_candidates_workspace_bytes(Q, L, d_q.numel(), 4096, C), dtype=torch.uint8, device=dev)
    ws_1 = torch.empty(tc.align_candidates_rates_workspace_bytes(Q, L, d_q.numel(), 1, 4096, C), dtype=torch.uint8, device=dev)
    out_0 = torch.empty((Q, C + 1, 2), dtype=torch.int32, device=dev)
    out_1 = torch.empty((Q, C + 1, 3), dtype=torch.int32, device=dev)
    plain = lambda: dc.align_candidates_block(d_q, d_off, L, c=C, min_count=2, cap=4096, out=out_0, workspace=ws_0)    # noqa: E731
    one = lambda: dc.align_candidates_rates_block(d_q, d_off, L, (1.0,), c=C, min_count=2, cap=4096, out=out_1,        # noqa: E731
                                                  workspace=ws_1)
    turns = [timed(fn, args.reps) for fn in (plain, one, plain, one)]
    same = bool((out_1.cpu().numpy()[:, :, :2] == out_0.cpu().numpy()).all())
    print(f"{Q:3d}   plain {stats(turns[0])}   rates {stats(turns[1])}   plain {stats(turns[2])}   rates {stats(turns[3])}   "
          f"columns 0..1 equal: {same}")
if args.turns_only:
    dc.close()
    sys.exit(0)
print()
print("ms per call, median (IQR)")
print(f"{'Q':>3s} {'R':>2s} {'cand R':>20s} {'cand+parts':>20s} {'sweep R (k=16)':>20s} {'true row first':>15s} "
      f"{'sweep has it':>13s} {'n_pairs median':>15s}")
for Q in (1, 16, 64):
    qs = queries[:Q]
    d_q, d_off, L = tc.pack_queries(qs, dev)
    for rates in RATE_LISTS:
        R = len(rates)
        ws_c = torch.empty(tc.align_candidates_rates_workspace_bytes(Q, L, d_q.numel(), R, 4096, C), dtype=torch.uint8, device=dev)
        ws_p = torch.empty(tc.align_parts_workspace_bytes(Q, L, d_q.numel(), C, 1), dtype=torch.uint8, device=dev)
        ws_s = torch.empty(tc.align_span_topk_workspace_bytes(Q, L, d_q.numel(), K), dtype=torch.uint8, device=dev)
        out_c = torch.empty((Q, C + 1, 3), dtype=torch.int32, device=dev)
        out_p = torch.empty((Q, C, 2, 6), dtype=torch.int32, device=dev)
        out_s = torch.empty((Q, K + 1, 8), dtype=torch.int32, device=dev)
        cand = lambda: dc.align_candidates_rates_block(d_q, d_off, L, rates, c=C, min_count=2, cap=4096, out=out_c,      # noqa: E731
                                                       workspace=ws_c)

        def both():
            cand()
            dc.align_parts_block(d_q, d_off, L, out_c[:, :C, 0], eps=EPS, rates=rates, min_votes=MIN_VOTES, max_parts=1, out=out_p,
                                 workspace=ws_p)
        sweep = lambda: dc.align_span_topk_block(d_q, d_off, L, eps=EPS, rates=rates, k=K, min_votes=MIN_VOTES, local=True,   # noqa: E731
                                                 out=out_s, workspace=ws_s)
        t_c, t_b = timed(cand, args.reps), timed(both, args.reps)
        t_s = timed(sweep, args.sweep_reps)
        block, swept = out_c.cpu().numpy(), out_s.cpu().numpy()
        first = sum(int(block[q, 0, 0]) == int(ids[src[q]]) and int(block[q, 0, 2]) == rates.index(SPEED) for q in range(Q))
        has = sum(int(swept[q, 0, 0]) == int(ids[src[q]]) for q in range(Q))
        print(f"{Q:3d} {R:2d} {stats(t_c):>20s} {stats(t_b):>20s} {stats(t_s):>20s} {first:>11d}/{Q:<3d} {has:>9d}/{Q:<3d} "
              f"{int(np.median(np.abs(block[:, C, 1]))):>15d}")
dc.close()
