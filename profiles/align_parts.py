#!/usr/bin/env python3
"""Every aligned part of named stored videos (tvz_align_parts) beside the search that names them
(tvz_align_span_topk), on the table and queries of profiles/align_span.py: 100k rows x ~200 cuts, stored rows of 200
cuts shifted by an hour, eps 1/30, k = 16, rates (1.0,).
   span    tvz_align_span_topk, TVZ_ALIGN_LOCAL, min_votes 8        (the existing call, timed in the same run)
   parts   tvz_align_parts on the ids of the block the search wrote at B = 2^22, taken by strides, min_votes 8,
           max_parts 1..4 (at B = 900 the search finds nothing - the copy is an hour away - so both widths walk the
           rows the wide search named; at B = 900 their part 0 stays below min_votes and the list is empty)
at B = 900 and B = 2^22, Q in (1, 16); device events around the enqueued call - whole calls: sort + locate + walk +
pick -, medians with IQR.  Before timing at B = 2^22, part 0 and the rate of every pair are checked against the hit
that named it (every id of the table stands once).  One process, one GPU:
   timeout -k 10 420 python3 profiles/align_parts.py > profiles/align_parts.txt"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rows", type=int, default=100_000)
args = ap.parse_args()

import torch  # noqa: E402

from tvidz_amd import _lib, corpus as tc, synth  # noqa: E402

dev = torch.device("cuda:0")
EPS, K, NQ, SHIFT, MIN_VOTES = 1.0 / 30, 16, 200, 3600.0, 8
RATES = (1.0,)
BS = {"B=900": 30.0, "B=2^22": tc.ALIGN_WIDE_MAX_B * EPS}
ids, offs, keys = synth.synth_timestamp_corpus(args.rows, seed=synth.CORPUS_SEED)
dc = tc.DeviceCorpus(0)
dc.upload_csr(ids, offs, keys)
lib = _lib.load()
rng = np.random.default_rng(synth.CORPUS_SEED + 7)
src = rng.permutation(np.flatnonzero(np.diff(offs) >= NQ))[:16].tolist()      # rows with at least NQ cuts
queries = [(keys[offs[r]:offs[r + 1]][:NQ] + SHIFT).tolist() for r in src]
stream = torch.cuda.current_stream(dev)
h_rates = (C.c_double * len(RATES))(*RATES)


def span(p, mo):
    d_q, d_off, longest, ws, block = p
    _lib.check(lib.tvz_align_span_topk(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, EPS, mo, h_rates,
                                       len(RATES), MIN_VOTES, 0, tc.ALIGN_LOCAL, None, K, block.data_ptr(), ws.data_ptr(),
                                       ws.numel(), stream.cuda_stream))


def parts(p, mo, P, out):
    d_q, d_off, longest, ws, block = p
    _lib.check(lib.tvz_align_parts(dc._h, d_q.data_ptr(), d_off.data_ptr(), d_off.numel() - 1, longest, block.data_ptr(), 8,
                                   (K + 1) * 8, K, EPS, mo, h_rates, len(RATES), MIN_VOTES, P, out.data_ptr(), ws.data_ptr(),
                                   ws.numel(), stream.cuda_stream))


def timed(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn(*a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(xs):
    q1, med, q3 = np.percentile(np.asarray(xs), [25, 50, 75])
    return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4)}


wide_block = {}
res = {"rows": args.rows, "query_len": NQ, "eps": EPS, "k": K, "min_votes": MIN_VOTES, "rates": list(RATES), "reps": args.reps,
       "ms_per_call": {}, "pairs": {}}
for bname, mo in reversed(list(BS.items())):                                  # the wide search first: it names the ids
    full = bname == "B=2^22"
    for nq in (1, 16):
        d_q, d_off, longest = tc.pack_queries(queries[:nq], dev)
        need = max(tc.align_span_topk_workspace_bytes(nq, longest, d_q.numel(), K),
                   tc.align_parts_workspace_bytes(nq, longest, d_q.numel(), K, 4))
        p = (d_q, d_off, longest, torch.empty(need, dtype=torch.uint8, device=dev),
             torch.empty((nq, K + 1, 8), dtype=torch.int32, device=dev))
        reps = max(3, args.reps // 4) if full else args.reps
        span(p, mo)                                                            # warm-up
        res["ms_per_call"][f"{bname} Q={nq} span"] = stats([timed(span, p, mo) for _ in range(reps)])
        if full:
            wide_block[nq] = p[4].clone()
        p = p[:4] + (wide_block[nq],)                                          # the ids of the wide search's block
        hits = p[4].cpu().numpy()
        for P in (1, 2, 3, 4):
            out = torch.empty((nq, K, 1 + P, 6), dtype=torch.int32, device=dev)
            parts(p, mo, P, out)                                               # warm-up, and the check
            got = out.cpu().numpy()
            named = 0
            for q in range(nq):
                for j in range(K):
                    vid, row_len, best_bin, votes, rate, t_first, t_last, nr = hits[q, j].tolist()
                    if vid < 0:
                        assert got[q, j, 0, 0] == -1
                        continue
                    named += 1
                    if not full:
                        assert got[q, j, 0].tolist()[:2] == [vid, row_len] and got[q, j, 0, 4] == 1
                        continue
                    assert got[q, j, 0].tolist() == [vid, row_len, rate, got[q, j, 0, 3], 1, NQ] and got[q, j, 0, 3] >= 1
                    assert got[q, j, 1].tolist() == [best_bin, votes, t_first, t_last, t_last - t_first + 1, nr]
            res["pairs"][f"{bname} Q={nq}"] = named
            res["ms_per_call"][f"{bname} Q={nq} parts P={P}"] = stats([timed(parts, p, mo, P, out) for _ in range(args.reps)])
res["checked"] = "at B = 2^22 part 0 and the rate of every named pair equal the span hit's columns"
print("ms per call, median (IQR); xN = tvz_align_span_topk / tvz_align_parts on the same batch")
for bname in BS:
    for nq in (1, 16):
        s = res["ms_per_call"][f"{bname} Q={nq} span"]
        cells = [f"span {s['median']:.4f} ({s['iqr']:.4f})"]
        for P in (1, 2, 3, 4):
            t = res["ms_per_call"][f"{bname} Q={nq} parts P={P}"]
            cells.append(f"P={P} {t['median']:.4f} ({t['iqr']:.4f}) x{s['median'] / t['median']:.1f}")
        print(f"{bname:7s} Q={nq:<3d} pairs={res['pairs'][f'{bname} Q={nq}']:<4d} " + "   ".join(cells))
print(json.dumps(res))
dc.close()
