#!/usr/bin/env python3
"""Candidate ids for LONG uploads (tvz_align_candidates_long) against the sweep, on the table of profiles/gap_candidates.py
(100k rows x ~200 cuts, synth_timestamp_corpus) with 64 stored videos of 1,500 cuts on a 30 fps grid upserted into it;
the uploads are those 64 shifted by an hour (eps 1/30, gap_eps 1/30):
   long        tvz_align_candidates_long alone, C = 16
   long+parts  ... followed by tvz_align_parts over the block's ids, max_parts = 1
   sweep       tvz_align_span_topk with TVZ_ALIGN_LOCAL at B = 2^22, k = 16, min_votes 8: what the Inspector takes for
               these uploads without near_candidates_long
each at Q = 1, 16, 64; device events around the enqueued calls, medians with IQR; how often the true row leads the block.
Then the plain tvz_align_candidates at Q = 1, 16, 64 on 200-cut uploads (profiles/gap_candidates.py's), for the
comparison of this build with its parent:  --plain-only --lib PATH  runs that part alone on another build of the
library (one without the new exports).  One process, one GPU:
   timeout -k 10 900 python3 profiles/gap_candidates_long.py > gap_candidates_long.txt"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--sweep-reps", type=int, default=3)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--lib", default=None)
args = ap.parse_args()

import torch  # noqa: E402

from tvidz_amd import _lib  # noqa: E402

if args.lib:                                                                      # another build: it has no long exports
    _lib.SO_PATH, _lib.GAP_LONG_SIGNATURES = os.path.abspath(args.lib), {}
from tvidz_amd import corpus as tc, synth  # noqa: E402

dev = torch.device("cuda:0")
EPS, GAP_EPS, K, C, NQ, NLONG, SHIFT, MIN_VOTES = 1.0 / 30, 1.0 / 30, 16, 16, 200, 1500, 3600.0, 8
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
rng = np.random.default_rng(synth.CORPUS_SEED + 11)
src = np.random.default_rng(synth.CORPUS_SEED + 7).permutation(np.flatnonzero(np.diff(offs) >= NQ))[:64].tolist()
short_queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src]
films = [(rng.integers(0, 3000) + np.concatenate([[0], np.cumsum(rng.integers(30, 241, size=NLONG - 1))])) / 30.0 for _ in range(64)]
FILM_ID = 50_000_000
print(f"gap candidates for long uploads: {args.rows} rows, {int(offs[-1])} keys, + 64 rows of {NLONG} cuts; eps {EPS:.4f}, gap_eps "
      f"{GAP_EPS:.4f}, library {_lib.SO_PATH}, {torch.cuda.get_device_name(0)}")


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
for i, f in enumerate(films):
    dc.upsert(FILM_ID + i, f)
dc.set_gap_index(GAP_EPS)
torch.cuda.synchronize()
print("gap_index_stats:", dc.gap_index_stats())

print()
print("tvz_align_candidates (the plain call), 200-cut uploads, C = 16: ms per call, median (IQR)")
for Q in (1, 16, 64):
    d_q, d_off, L = tc.pack_queries(short_queries[:Q], dev)
    ws = torch.empty(tc.align_candidates_workspace_bytes(Q, L, d_q.numel(), 4096, C), dtype=torch.uint8, device=dev)
    out = torch.empty((Q, C + 1, 2), dtype=torch.int32, device=dev)
    t = timed(lambda: dc.align_candidates_block(d_q, d_off, L, c=C, min_count=2, cap=4096, out=out, workspace=ws), args.reps)
    print(f"{Q:3d} {stats(t):>20s}")
if args.plain_only:
    dc.close()
    sys.exit(0)

print()
print(f"{NLONG}-cut uploads: ms per call, median (IQR)")
print(f"{'Q':>3s} {'long':>20s} {'long+parts':>20s} {'sweep (k=16)':>20s} {'true row first':>15s} {'candidates':>11s} {'workspace MiB':>14s}")
for Q in (1, 16, 64):
    qs = [(f + SHIFT).tolist() for f in films[:Q]]
    d_q, d_off, L = tc.pack_queries(qs, dev)
    need = tc.align_candidates_long_workspace_bytes(Q, L, d_q.numel(), 4096, C)
    ws_c = torch.empty(need, dtype=torch.uint8, device=dev)
    ws_p = torch.empty(tc.align_parts_workspace_bytes(Q, L, d_q.numel(), C, 1), dtype=torch.uint8, device=dev)
    ws_s = torch.empty(tc.align_span_topk_workspace_bytes(Q, L, d_q.numel(), K), dtype=torch.uint8, device=dev)
    out_c = torch.empty((Q, C + 1, 2), dtype=torch.int32, device=dev)
    out_p = torch.empty((Q, C, 2, 6), dtype=torch.int32, device=dev)
    out_s = torch.empty((Q, K + 1, 8), dtype=torch.int32, device=dev)
    cand = lambda: dc.align_candidates_long_block(d_q, d_off, L, c=C, min_count=2, cap=4096, out=out_c, workspace=ws_c)   # noqa: E731

    def both():
        cand()
        dc.align_parts_block(d_q, d_off, L, out_c[:, :C, 0], eps=EPS, min_votes=MIN_VOTES, max_parts=1, out=out_p, workspace=ws_p)
    sweep = lambda: dc.align_span_topk_block(d_q, d_off, L, eps=EPS, k=K, min_votes=MIN_VOTES, local=True, out=out_s,    # noqa: E731
                                             workspace=ws_s)
    t_c, t_b, t_s = timed(cand, args.reps), timed(both, args.reps), timed(sweep, args.sweep_reps)
    block, parts, swept = out_c.cpu().numpy(), out_p.cpu().numpy(), out_s.cpu().numpy()
    first = sum(int(block[q, 0, 0]) == FILM_ID + q for q in range(Q))
    votes = sum(int(parts[q, 0, 1, 1]) == NLONG for q in range(Q))
    swept_first = sum(int(swept[q, 0, 0]) == FILM_ID + q for q in range(Q))
    print(f"{Q:3d} {stats(t_c):>20s} {stats(t_b):>20s} {stats(t_s):>20s} {first:>11d}/{Q:<3d} {int(np.median(np.abs(block[:, C, 1]))):>11d} "
          f"{need / 2**20:>14.1f}")
    print(f"        part 0 of the true row holds all {NLONG} votes: {votes}/{Q}; the sweep's first row is the true row: {swept_first}/{Q}; "
          f"overflowed lists: {int((block[:, C, 1] < 0).sum())}; sweep / long+parts = {np.median(t_s) / np.median(t_b):.0f}x")
dc.close()
