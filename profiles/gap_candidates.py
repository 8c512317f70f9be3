#!/usr/bin/env python3
"""Candidate ids from the gap index against the sweep, on the table and queries of profiles/align_wide_topk.py (100k rows
x ~200 cuts, synth_timestamp_corpus; queries = stored rows of 200 cuts shifted by an hour; eps 1/30):
   cand        tvz_align_candidates alone, C = 16 and 64
   cand+parts  ... followed by tvz_align_parts over the block's ids, max_parts = 1
   sweep       tvz_align_span_topk with TVZ_ALIGN_LOCAL at B = 2^22, k = 16, the same batch, the same run
each at Q = 1, 16, 64; device events around the enqueued calls, medians with IQR.  Also: the share of queries whose K =
16 best ids by the local score are the same from both paths (all of them with at least 8 votes, and those that score
at least 0.5: what a report with a threshold keeps); the time and the device bytes of tvz_corpus_gap_index on
the populated handle; the host time of tvz_corpus_upsert with and without gap codes.  One process, one GPU:
   timeout -k 10 900 python3 profiles/gap_candidates.py > gap_candidates.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--sweep-reps", type=int, default=3)
ap.add_argument("--upserts", type=int, default=1000)
args = ap.parse_args()

import torch  # noqa: E402

from tvidz_amd import corpus as tc, synth  # noqa: E402

dev = torch.device("cuda:0")
EPS, GAP_EPS, K, NQ, SHIFT, MIN_VOTES = 1.0 / 30, 1.0 / 30, 16, 200, 3600.0, 8
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()          # rows with at least NQ cuts
queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src]
print(f"gap candidates: {args.rows} rows, {int(offs[-1])} keys, queries of {NQ} cuts shifted by {SHIFT:g} s, eps {EPS:.4f}, "
      f"gap_eps {GAP_EPS:.4f}, {torch.cuda.get_device_name(0)}")


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return f"{med:9.4f} ({q3 - q1:.4f})"


def upserts(dc, first_id, n):
    """host time of n upserts of new ids, 200 cuts each: what the caller waits for (the device work is stream-ordered)"""
    rows = [np.sort(rng.uniform(0.0, 7200.0, size=NQ)) for _ in range(n)]
    t = []
    for i, r in enumerate(rows):
        t0 = time.perf_counter()
        dc.upsert(first_id + i, r)
        t.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    t = np.asarray(t)
    return f"median {np.median(t):8.1f} us, mean {t.mean():8.1f} us, max {t.max():9.1f} us over {n}"


free_start = torch.cuda.mem_get_info(0)[0]
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
torch.cuda.synchronize()
print(f"the handle and its index after the upload: {(free_start - torch.cuda.mem_get_info(0)[0]) / 2**20:.1f} MiB of device memory, "
      f"{dc.index_stats()}")
dc.upsert(10_000_000, queries[0])                                                 # warm
print("tvz_corpus_upsert without gap codes:", upserts(dc, 20_000_000, args.upserts))
free0 = torch.cuda.mem_get_info(0)[0]
t0 = time.perf_counter()
dc.set_gap_index(GAP_EPS)
torch.cuda.synchronize()
t_ix = time.perf_counter() - t0
free1 = torch.cuda.mem_get_info(0)[0]
st = dc.gap_index_stats()
print(f"tvz_corpus_gap_index on the populated handle: {t_ix * 1e3:.1f} ms (host wall, the call synchronises), "
      f"{(free0 - free1) / 2**20:.1f} MiB of device memory, {st['rows']} rows, {st['codes']} codes")
print("tvz_corpus_upsert with gap codes:   ", upserts(dc, 30_000_000, args.upserts))
print("gap_index_stats:", dc.gap_index_stats())
stream = torch.cuda.current_stream(dev)


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


def best_ids(rows8, m, min_score=0):
    """the K best ids of span rows (video_id, row_len, bin, votes, rate, t_first, t_last, nr) by the local order, of those
    that score at least min_score (20-bit fixed point)"""
    rows8 = [tuple(int(x) for x in r) for r in rows8 if r[0] >= 0 and r[3] >= MIN_VOTES]
    keyed = sorted((tc.align_span_order_key(r, m, local=True), r[0]) for r in rows8)
    return [vid for key, vid in keyed[:K] if -key[0] >= min_score]


print()
print("ms per call, median (IQR)")
print(f"{'Q':>3s} {'C':>3s} {'cand':>20s} {'cand+parts':>20s} {'sweep (k=16)':>20s} {'same K best':>12s} {'... scoring >= 0.5':>19s} {'true row first':>15s}")
for Q in (1, 16, 64):
    qs = queries[:Q]
    d_q, d_off, L = tc.pack_queries(qs, dev)
    ws_s = torch.empty(tc.align_span_topk_workspace_bytes(Q, L, d_q.numel(), K), dtype=torch.uint8, device=dev)
    out_s = torch.empty((Q, K + 1, 8), dtype=torch.int32, device=dev)
    sweep = lambda: dc.align_span_topk_block(d_q, d_off, L, eps=EPS, k=K, min_votes=MIN_VOTES, local=True, out=out_s,    # noqa: E731
                                             workspace=ws_s)
    t_sweep = timed(sweep, args.sweep_reps)
    swept = out_s.cpu().numpy()
    for C in (16, 64):
        ws_c = torch.empty(tc.align_candidates_workspace_bytes(Q, L, d_q.numel(), 4096, C), dtype=torch.uint8, device=dev)
        ws_p = torch.empty(tc.align_parts_workspace_bytes(Q, L, d_q.numel(), C, 1), dtype=torch.uint8, device=dev)
        out_c = torch.empty((Q, C + 1, 2), dtype=torch.int32, device=dev)
        out_p = torch.empty((Q, C, 2, 6), dtype=torch.int32, device=dev)
        cand = lambda: dc.align_candidates_block(d_q, d_off, L, c=C, min_count=2, cap=4096, out=out_c, workspace=ws_c)   # noqa: E731

        def both():
            cand()
            dc.align_parts_block(d_q, d_off, L, out_c[:, :C, 0], eps=EPS, min_votes=MIN_VOTES, max_parts=1, out=out_p, workspace=ws_p)
        t_c, t_b = timed(cand, args.reps), timed(both, args.reps)
        parts, block = out_p.cpu().numpy(), out_c.cpu().numpy()
        same = half = first = 0
        missing = []                                                              # votes of the sweep's ids the candidates lack
        for q in range(Q):
            rows8 = [(p[0][0], p[0][1], p[1][0], p[1][1], p[0][2], p[1][2], p[1][3], p[1][5]) for p in parts[q] if p[0][3] >= 1]
            a, b = best_ids(rows8, NQ), best_ids(swept[q, :K], NQ)
            same += a == b
            half += best_ids(rows8, NQ, 1 << 19) == best_ids(swept[q, :K], NQ, 1 << 19)
            missing += [int(r[3]) for r in swept[q, :K] if r[0] >= 0 and r[3] >= MIN_VOTES and int(r[0]) not in a]
            first += int(block[q, 0, 0]) == int(ids[src[q]])
        print(f"{Q:3d} {C:3d} {stats(t_c):>20s} {stats(t_b):>20s} {stats(t_sweep):>20s} {same:>8d}/{Q:<3d} {half:>15d}/{Q:<3d} {first:>11d}/{Q:<3d}")
        if missing:
            print(f"        the sweep's ids the candidate path lacks: {len(missing)} over {Q} queries, votes {min(missing)}..{max(missing)} "
                  f"(the true row: {NQ}); candidates per query: median {int(np.median(np.abs(block[:, C, 1])))}")
dc.close()
