#!/usr/bin/env python3
"""tvz_align_parts beside tvz_align_parts_flags with TVZ_ALIGN_TWO_BINS on the workload of profiles/align_parts.py: 100k
rows x ~200 cuts, queries of 200 cuts shifted by an hour, eps 1/30, k = 16, rates (1.0,), min_votes 8; the ids are those
of the span search's block at B = 2^22, taken by strides.
   cells   Q in (1, 16) x B in (900, 2^22) x max_parts in (1, 2); whole calls (sort + locate + walk + pick), device
           events around the enqueued call, the median of --reps calls per cell
   legs    the two exports ALTERNATE, one fresh process per leg (single, two, single, two, ...), --rounds rounds: the
           table, the search and the warm-up are made anew in every leg, on one GPU, one build
   report  per cell the median over the rounds of either export, the rounds' range, and the ratio two / single; a ratio
           is marked where the two exports' ranges over the rounds do not overlap
Before timing, every leg checks its part 0 against the span search's hit (the single-bin export; the two-bin one against
the two-bin search's hit on the same ids).
   timeout -k 10 900 python3 profiles/align_parts_two_bins.py > profiles/align_parts_two_bins.txt"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--leg", choices=("single", "two"), default=None)
args = ap.parse_args()

EPS, K, NQ, SHIFT, MIN_VOTES = 1.0 / 30, 16, 200, 3600.0, 8
RATES = (1.0,)
CELLS = [(nq, bname, P) for bname in ("B=900", "B=2^22") for nq in (1, 16) for P in (1, 2)]


def leg(which):
    import torch

    from tvidz_amd import _lib, corpus as tc, synth

    dev = torch.device("cuda:0")
    BS = {"B=900": 30.0, "B=2^22": tc.ALIGN_WIDE_MAX_B * EPS}
    ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
    dc = tc.DeviceCorpus(0)
    dc.upload_csr(ids, offs, keys)
    lib = _lib.load()
    rng = np.random.default_rng(synth.CORPUS_SEED + 7)
    src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:16].tolist()
    queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src]
    stream = torch.cuda.current_stream(dev)
    h_rates = (C.c_double * len(RATES))(*RATES)
    two = which == "two"

    def parts(p, mo, P, out):
        d_q, d_off, longest, ws, block = p
        front = (dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, block.data_ptr(), 8, (K + 1) * 8, K, EPS, mo,
                 h_rates, len(RATES), MIN_VOTES, P)
        back = (out.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream)
        _lib.check(lib.tvz_align_parts_flags(*front, tc.ALIGN_TWO_BINS, *back) if two else lib.tvz_align_parts(*front, *back))

    def timed(fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(*a)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    out_ms = {}
    for nq in (1, 16):
        d_q, d_off, longest = tc.pack_queries(queries[:nq], dev)
        need = max(tc.align_span_topk_workspace_bytes(nq, longest, d_q.numel(), K),
                   tc.align_parts_workspace_bytes(nq, longest, d_q.numel(), K, 4))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        # the ids: the single-bin span search at any shift, for both legs; the hit to check against: this leg's search
        named = dc.align_span_topk_block(d_q, d_off, longest, eps=EPS, rates=RATES, k=K, min_votes=MIN_VOTES, local=True, workspace=ws)
        hits = named if not two else dc.align_span_topk_block(d_q, d_off, longest, eps=EPS, rates=RATES, k=K, min_votes=1,
                                                                 two_bins=True, workspace=ws)
        by_id = {(q, int(r[0])): r.tolist() for q, rows in enumerate(hits.cpu().numpy()) for r in rows[:K] if r[0] >= 0}
        p = (d_q, d_off, longest, ws, named)
        for bname, mo in BS.items():
            for P in (1, 2):
                out = torch.empty((nq, K, 1 + P, 6), dtype=torch.int32, device=dev)
                parts(p, mo, P, out)                                           # warm-up, and the check
                if bname == "B=2^22":
                    got, ids_h, checked = out.cpu().numpy(), named.cpu().numpy()[:, :K, 0], 0
                    for q in range(nq):
                        for j in range(K):
                            hit = by_id.get((q, int(ids_h[q, j])))
                            if ids_h[q, j] < 0 or hit is None or got[q, j, 0, 3] < 1:
                                continue
                            checked += 1
                            assert got[q, j, 1].tolist()[:4] == [hit[2], hit[3], hit[5], hit[6]], (which, q, j)
                    assert checked >= nq, (which, checked)
                ms = [timed(parts, p, mo, P, out) for _ in range(args.reps)]
                out_ms[f"{bname} Q={nq} P={P}"] = float(np.median(ms))
    dc.close()
    print("LEG " + json.dumps({"which": which, "ms": out_ms}))


if args.leg:
    leg(args.leg)
    sys.exit(0)

runs = {"single": [], "two": []}
for _ in range(args.rounds):
    for which in ("single", "two"):                                             # alternate; a fresh process per leg
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", which, "--reps", str(args.reps), "--rows", str(args.rows)],
                           capture_output=True, text=True, timeout=280, stdin=subprocess.DEVNULL)
        if r.returncode != 0:                                                   # nothing more is started on the GPU
            sys.exit(f"leg {which} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
        runs[which].append(json.loads(line[4:])["ms"])
print(f"ms per call: median over {args.rounds} rounds [the rounds' range], each round the median of {args.reps} calls; "
      "ratio = two bins / single bin; * = the two ranges do not overlap")
res = {"rows": args.rows, "query_len": NQ, "eps": EPS, "k": K, "min_votes": MIN_VOTES, "reps": args.reps, "rounds": args.rounds,
       "cells": {}}
for nq, bname, P in CELLS:
    cell = f"{bname} Q={nq} P={P}"
    s, t = [r[cell] for r in runs["single"]], [r[cell] for r in runs["two"]]
    apart = min(t) > max(s) or max(t) < min(s)
    ratio = float(np.median(t) / np.median(s))
    res["cells"][cell] = {"single": s, "two": t, "ratio": round(ratio, 4), "beyond_spread": bool(apart)}
    print(f"{bname:7s} Q={nq:<3d} P={P}  tvz_align_parts {np.median(s):8.4f} [{min(s):.4f} .. {max(s):.4f}]   "
          f"tvz_align_parts_flags|TWO_BINS {np.median(t):8.4f} [{min(t):.4f} .. {max(t):.4f}]   x{ratio:.3f}{' *' if apart else ''}")
print(json.dumps(res))
