"""Randomised differential cases for the near-duplicate search: every alignment and candidate call of the library
against the plain references under tests/, whole blocks, bit for bit.

Shared by tests/test_near_fuzz_gpu.py (a seeded, bounded slice inside the `-m gpu` suite), by
tests/test_near_fuzz_cases_cpu.py (the generator and the references alone: determinism, contract, counters and the
perturbed references the cases must tell from the right ones) and by `profiles/fuzz_parity.py --family near` (the soak).

  gen_case(rng)            one case as plain data: a table, a batch of uploads and a list of steps (gap index, upload,
                           calls, upserts, build_index, a sharded round).  Every random draw happens here, from the one
                           np.random.default_rng(seed) of cases(); nothing drawn depends on an answer.
  Expect(case, refs)       the host's picture of the table (db.py's first-row rule for upserts) and the expected block
                           of every call, from `refs` - REFS: the references as they stand; a test swaps single entries
                           for perturbed wrappers.  The ids of a parts call come from the expected span or candidates
                           block of the same case.
  walk(seed, max_cases)    generator + references, no device: yields (case index, step index, call, expected blocks).
  run(seed, max_cases)     the same walk with every call made on the device (device=None: references alone) -> counters;
                           AssertionError(("NEAR MISMATCH", dict(seed=, case=, call=, qi=, ...))) at the first difference.

The relations between forms that include/tvz.h states need no reference and run on the device beside every call they
apply to: wide == bounded for B <= 2047 without flags; rates (1.0,) == wide in columns 0..3; span == rates in columns
0..4 without TVZ_ALIGN_LOCAL; candidates_rates (1.0,) == candidates over distinct ids; a ShardedCorpus of R shards ==
the one handle (the candidate calls: where no list, a shard's or the one handle's, went beyond cap); the device merges == the host merges of tvidz_amd/corpus.py and the references' merge_ref.

Counters come from the inputs and the references' outputs alone, never from the library's answer."""
import hashlib
import json
import math
import time
from types import SimpleNamespace

import numpy as np

from tests import (align_parts_ref as apr, align_parts_two_bins_ref as apf, align_rates_ref as arr, align_ref as ar,
                   align_span_ref as asr, align_topk_ref as atr, align_two_bins_ref as atb, align_wide_ref as awr,
                   gap_candidates_rates_ref as gcrr, gap_candidates_ref as gcr)
from tvidz_amd import corpus as tc

SPECIAL = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324, 1e300, 1.5, 0.1 + 0.2, 0.3])     # fuzz_cases.SPECIAL
EPS = (0.1, 1 / 30, 1 / 24, 1 / 64, 1e-3)
GRIDS = (1 / 24, 1 / 25, 1 / 30, 1001 / 30000)
RATES = (1.0, 0.96, 25 / 24, 24 / 25, 1001 / 1000, 1000 / 1001, 1.25, 0.8, 2.0)
ROW_LENS = (0, 1, 2, 3, 4, 63, 64, 65, 150)
GAP_EPS = (0.005, 0.02, 0.1)
WINDOW = 1024                                   # bins of one window of the walk (include/tvz.h, tvz_align_wide_topk: Cost)
ONE_WINDOW_B = 2047                             # B up to here is one window of all bins
RESUME_KEYS = 512                               # a row's first keys that have resume positions
GAP_DELTA_ROWS = 512                            # include/tvz.h: the delta table of an index is rebuilt from this many rows
REFUSED = atr.REFUSED
TOPK_FORMS = {"topk": tc.FORM_BOUNDED, "wide": tc.FORM_WIDE, "rates": tc.FORM_RATES, "span": tc.FORM_SPAN}
FORMS = ("topk", "wide", "wide_contain", "wide_two_bins", "rates", "span", "span_local", "parts", "parts_flags",
         "candidates", "candidates_rates", "shards", "merges")

REFS = SimpleNamespace(align=ar.align_ref, wide=awr.align_wide_ref, rates=arr.align_rates_ref, span=asr.align_span_ref,
                       two_bins=atb.align_two_bins_ref, parts=apr.align_parts_ref, parts_flags=apf.align_parts_flags_ref,
                       candidates=gcr.candidates, candidates_rates=gcrr.candidates_rates)


def refs_with(**swapped):
    """REFS with single entries replaced (the perturbed wrappers of tests/test_near_fuzz_cases_cpu.py)."""
    return SimpleNamespace(**{**vars(REFS), **swapped})


# ---------------------------------------------------------------------------------------------------- the generator
def offset_for(B, eps):
    """A max_offset whose B = floor(max_offset / eps + 0.5) is exactly `B`."""
    mo = float(B) * eps
    for cand in (mo, np.nextafter(mo, np.inf), np.nextafter(mo, -np.inf)):
        if cand >= 0.0 and awr.n_bins(eps, float(cand)) == B:
            return float(cand)
    raise AssertionError((B, eps))


def nudge(x, ulps):
    x = np.float64(x)
    for _ in range(abs(int(ulps))):
        x = np.nextafter(x, np.inf if ulps > 0 else -np.inf)
    return float(x)


def _draw_B(rng, big):
    """-> (kind, B or None for the widest): 0; one window; a few windows with 2B + 1 = 1 or 1023 mod 1024 (2B + 1 is
    odd: the last window of the walk holds one bin, or all but one) or anything else; the widest."""
    kind = str(rng.choice(["zero", "one", "multi", "multi_edge", "widest"], p=[0.08, 0.42, 0.22, 0.18, 0.10]))
    if kind == "zero":
        return kind, 0
    if kind == "one":
        return kind, int(rng.choice([1, 2, 7, 100, 1000, 2046, 2047, int(rng.integers(1, 2048))]))
    if kind == "multi":
        return kind, int(rng.integers(2048, 20000 if big else 6000))
    if kind == "multi_edge":
        j = int(rng.integers(4, 12))
        return kind, 512 * j - int(rng.integers(0, 2))                # 2B + 1 = 1024 j + 1, or 1024 j - 1
    return kind, None


def _cuts(rng, n, span, grid):
    if n == 0:
        return np.zeros(0)
    t0 = rng.uniform(0.0, span)
    if grid is None:
        return t0 + np.cumsum(rng.uniform(0.04, 6.0, n))
    return (int(t0 / grid) + np.cumsum(rng.integers(1, 150, n))) * grid


def _specials(rng, a, p=0.02):
    a = np.array(a, dtype=np.float64)
    m = rng.random(a.size) < p
    a[m] = SPECIAL[rng.integers(0, len(SPECIAL), int(m.sum()))]
    return a


def _edge_bins(rng, B, n):
    """n bins m whose upper edge (m + 1/2) eps a shift is put on: anywhere in the range, at its ends, and - beyond one
    window - the last slot of a window of the walk, (m + B) % 1024 == 1023."""
    Bm = min(B, 60000)
    out = []
    for _ in range(n):
        u = rng.random()
        if B > ONE_WINDOW_B and u < 0.5:
            out.append(-B + WINDOW - 1 + WINDOW * int(rng.integers(0, (2 * B + 1) // WINDOW)))
        elif u < 0.65:
            out.append(int(rng.choice([-B - 1, -B, B - 1, B])))
        else:
            out.append(int(rng.integers(-Bm, Bm + 1)))
    return [m for m in out if -B - 1 <= m <= B]


def _shift(rng, B, eps, where):
    """a shift t (stored = upload + t) inside the offset range, outside it, at its end, or on a bin's edge"""
    Bm = min(B, 60000)
    if where == "in":
        return float(rng.uniform(-Bm * eps, Bm * eps)) if rng.random() < 0.5 else int(rng.integers(-Bm, Bm + 1)) * eps
    if where == "out":
        return float(rng.choice([-1, 1])) * (B + int(rng.integers(1, 40)) + float(rng.random())) * eps
    if where == "end":
        return nudge(float(rng.choice([-1, 1])) * (B + float(rng.choice([0.0, 0.5]))) * eps, int(rng.integers(-4, 5)))
    m = (_edge_bins(rng, B, 1) or [0])[0]
    return nudge((m + 0.5) * eps, int(rng.integers(-4, 5)))


UPLOAD_KINDS = ("shift_in", "shift_out", "shift_end", "bin_edge", "scaled", "scaled_other", "excerpt", "compilation",
                "drop_insert", "jitter", "retime", "mirror", "random", "empty", "nan", "inf_zero", "tiny", "long_copy")
UPLOAD_P = np.array([10, 3, 4, 10, 7, 3, 9, 12, 6, 7, 6, 5, 3, 2, 2, 3, 5, 3], dtype=np.float64)


def _upload(rng, kind, rows, B, eps, rates, span):
    """One upload of `kind`, derived from the stored rows so that votes exist."""
    full = [np.asarray(k, dtype=np.float64) for _, k in rows if len(k) >= 4] or \
        [np.asarray(k, dtype=np.float64) for _, k in rows if len(k)] or [np.array([1.0, 2.5, 4.0, 7.5, 9.0])]
    row = np.sort(full[int(rng.integers(0, len(full)))][:160])
    if kind in ("shift_in", "shift_out", "shift_end", "bin_edge"):
        return row - _shift(rng, B, eps, kind.split("_", 1)[1] if kind != "bin_edge" else "edge")
    if kind in ("scaled", "scaled_other"):
        rho = float(rng.choice(rates)) if kind == "scaled" else float(rng.choice([0.9, 1.1, 24000 / 23976, 1.5]))
        return (row - _shift(rng, B, eps, str(rng.choice(["in", "edge"])))) / rho
    if kind == "excerpt":
        n = max(1, int(row.size * rng.uniform(0.1, 0.5)))
        a = int(rng.integers(0, row.size - n + 1))
        return row[a:a + n] - _shift(rng, B, eps, str(rng.choice(["in", "edge"])))
    if kind == "compilation":
        # excerpts of two or three rows - or two parts of ONE row, a scene taken out or an ad put in - back to back
        same = rng.random() < 0.6
        parts, at = [], float(rng.uniform(0.0, 5.0))
        for i in range(int(rng.integers(2, 4))):
            src = row if same else np.sort(full[int(rng.integers(0, len(full)))][:160])
            n = max(1, int(src.size * rng.uniform(0.1, 0.4)))
            a = int(rng.integers(0, src.size - n + 1))
            if same:
                a = min(src.size - n, (i * src.size) // 3)
            seg = src[a:a + n]
            t = seg[0] - at
            if np.isfinite(t) and rng.random() < 0.7:
                t = math.floor(t / eps) * eps + (0.0 if rng.random() < 0.5 else 0.5 * eps)     # on a bin, or on its edge
            with np.errstate(invalid="ignore"):
                moved = seg - t
            parts.append(moved)
            fin = moved[np.isfinite(moved)]
            at = (float(fin.max()) if fin.size else at) + float(rng.uniform(0.5, 20.0))
        return np.concatenate(parts)
    if kind == "drop_insert":
        keep = row[rng.random(row.size) > 0.1]
        extra = rng.uniform(0.0, span, int(rng.integers(1, 6)))
        return np.sort(np.concatenate([keep, extra])) - _shift(rng, B, eps, "in")
    if kind == "jitter":
        return row - _shift(rng, B, eps, str(rng.choice(["in", "edge"]))) + rng.uniform(-eps / 2, eps / 2, row.size)
    if kind == "retime":
        fps = float(rng.choice([24.0, 25.0, 30.0]))
        with np.errstate(invalid="ignore", over="ignore"):
            return np.round((row - _shift(rng, B, eps, "in")) * fps) / fps
    if kind == "mirror":
        # two values at the same distance on either side of stored keys: votes for +b and for -b alike
        c = row[np.isfinite(row)][:3]
        d = int(rng.integers(0, max(min(B, 40), 1) + 1)) * eps
        return np.concatenate([c - d, c + d]) if c.size else np.zeros(0)
    if kind == "random":
        return _cuts(rng, int(rng.choice([5, 30, 80])), span, None if rng.random() < 0.5 else float(rng.choice(GRIDS)))
    if kind == "empty":
        return np.zeros(0)
    if kind == "nan":
        return np.full(int(rng.integers(1, 6)), np.nan)
    if kind == "inf_zero":
        return np.concatenate([[np.inf, -np.inf, 0.0, -0.0, 5e-324], row[:int(rng.integers(0, 6))]])
    if kind == "tiny":
        n = int(rng.integers(1, 4))
        return row[:n] - _shift(rng, B, eps, "in")
    if kind == "long_copy":
        longest = max(full, key=len)
        return np.sort(longest) - _shift(rng, B, eps, "in")
    raise AssertionError(kind)


def _topk_call(rng, form, ids, Q):
    """the parameters of one top-k call of `form` (topk / wide / rates / span); the flags by the form table"""
    p = dict(form=form, k=int(rng.choice([1, 3, 16, 64])), min_votes=int(rng.choice([1, 2, 5])),
             min_score=int(rng.choice([0, 0, 1 << 18, (1 << 20) - 1, 1 << 20])), contain=False, local=False, two_bins=False,
             exclude_ids=None if rng.random() < 0.5 else [int(rng.choice(ids + [-1, 987654])) for _ in range(Q)])
    f = TOPK_FORMS[form]
    if f.flags:
        kind = int(rng.integers(0, 3 if "local" in f.flags else 2))          # contain and local together are refused
        p["contain"], p["local"] = kind == 1, kind == 2
        p["two_bins"] = bool(rng.random() < 0.5)
    return p


def _parts_call(rng, form, ids, Q, gap_on):
    """a parts call: where its ids come from (a span block, a candidates block, drawn at random) and its parameters"""
    src = str(rng.choice(["span", "candidates", "random"] if gap_on else ["span", "random"]))
    kmax = max(1, 24 // Q)
    p = dict(form=form, src=src, min_votes=int(rng.choice([1, 2, 5])), max_parts=int(rng.integers(1, 5)))
    if src == "span":
        p["span"] = dict(_topk_call(rng, "span", ids, Q), k=int(rng.choice([1, 3, 16])), min_score=0)
        p["step"] = int(rng.choice([1, 2]))
        p["k"] = min(kmax, -(-p["span"]["k"] // p["step"]))
    elif src == "candidates":
        c = int(rng.choice([1, 4, 16, 64]))
        p["cand"] = dict(form="candidates", c=c, min_count=int(rng.choice([1, 2])), cap=4096, exclude_ids=None)
        p["step"] = int(rng.choice([1, 2]))
        p["k"] = min(kmax, -(-c // p["step"]))
    else:
        k = int(rng.integers(1, kmax + 1))
        p["ids"] = [[int(rng.choice(ids + ids + [-1, 987654])) for _ in range(k)] for _ in range(Q)]
        p["transposed"] = bool(rng.random() < 0.5)                            # a [k, Q] tensor passed as its [Q, k] view
        p["k"] = k
    return p


def _cand_call(rng, form, ids, Q):
    c = int(rng.choice([1, 4, 16, 64]))
    return dict(form=form, c=c, min_count=int(rng.choice([1, 2, 4])), cap=max(int(rng.choice([1, 5, 4096])), c),
                exclude_ids=None if rng.random() < 0.5 else [int(rng.choice(ids + [-1])) for _ in range(Q)])


def _calls(rng, n, ids, Q, gap_on, cheap=False):
    forms = ["topk", "wide", "wide", "rates", "span", "span", "parts", "parts_flags"] + \
        (["candidates", "candidates_rates"] if gap_on else [])
    if cheap:                                   # a table of many rows: the vectorised references only
        forms = ["topk", "wide", "candidates", "candidates_rates"]
    out = []
    for form in rng.choice(forms, size=min(n, len(forms)), replace=False).tolist():
        if form in TOPK_FORMS:
            p = _topk_call(rng, form, ids, Q)
            if cheap:
                p["two_bins"] = False
            out.append(p)
        elif form in ("parts", "parts_flags"):
            out.append(_parts_call(rng, form, ids, Q, gap_on))
        else:
            out.append(_cand_call(rng, form, ids, Q))
    return [dict(op="call", **p) for p in out]


def gen_case(rng, big=False):
    """One case as plain data.  `big` (the soak): more rows, longer rows, wider ranges."""
    eps = float(rng.choice(EPS))
    b_kind, B = _draw_B(rng, big)
    max_offset = None if B is None else offset_for(B, eps)
    B = tc.ALIGN_WIDE_MAX_B if B is None else B
    n_rates = int(rng.choice([1, 1, 2, 3, 4, 8]))
    rates = [float(x) for x in rng.choice(RATES, size=n_rates, replace=False)]
    if n_rates > 1 and rng.random() < 0.4:
        rates[int(rng.integers(1, n_rates))] = rates[0]                       # an entry twice: the tie goes to the smaller index
    if rng.random() < 0.5:
        rates = rates[::-1]
    gap_eps = float(rng.choice(GAP_EPS))
    span = float(rng.choice([30.0, 300.0, 3000.0]))
    # ---- the table
    n_rows = int(rng.choice([1, 2, 5, 12, 30, 80] + ([200, 400] if big else []),
                            p=None if big else [0.08, 0.12, 0.25, 0.27, 0.20, 0.08]))
    grid_rows = bool(rng.random() < 0.6)
    rows, per_id = [], {}
    for r in range(n_rows):
        n = int(rng.choice(ROW_LENS + ((300, 500) if big else ()), p=None if big else
                           [0.05, 0.08, 0.08, 0.08, 0.19, 0.12, 0.12, 0.12, 0.16]))
        keys = _specials(rng, _cuts(rng, n, span, float(rng.choice(GRIDS)) if grid_rows else None))
        if n >= 3 and rng.random() < 0.15:
            keys = np.concatenate([keys, keys[:3]])                           # repeated keys
        if rng.random() < 0.3:
            keys = rng.permutation(keys)
        vid = int(rng.integers(1, max(2, int(n_rows * 0.8)) + 1))
        if per_id.get(vid, 0) >= tc.ALIGN_PARTS_MAX_ROWS:
            vid = 1000 + r
        per_id[vid] = per_id.get(vid, 0) + 1
        rows.append((vid, keys))
    for _ in range(n_rows // 8):                                              # duplicate rows
        a, b = rng.integers(0, n_rows, 2)
        rows[b] = (rows[b][0], rows[a][1].copy())
    if rng.random() < 0.22:                                                   # beyond the 512 resume positions
        n = int(rng.integers(RESUME_KEYS + 1, 701))
        rows[int(rng.integers(0, n_rows))] = (2000, _cuts(rng, n, span / 4, float(rng.choice(GRIDS))
                                                         if grid_rows or rng.random() < 0.5 else None))
    # rows made FROM an upload, so that the pair's quotient lies on a bin's edge to the last bit: keys within 4 ulps of
    # (m + 1/2) eps against an upload value of 0.0, and the anchor upload at one of the rates, moved by (m + 1/2) eps
    anchor = None
    if rng.random() < 0.45:
        ms = _edge_bins(rng, B, 24)
        rows.append((3000, np.array([nudge((m + 0.5) * eps, int(rng.integers(-4, 5))) for m in ms])))
        anchor = np.sort(_cuts(rng, int(rng.integers(12, 40)), span, float(rng.choice(GRIDS))))
        rho = float(rates[int(rng.integers(0, len(rates)))])
        m = (_edge_bins(rng, B, 1) or [0])[0]
        rows.append((3001, np.array([nudge(x, 0 if rng.random() < 0.7 else int(rng.integers(-2, 3)))
                                     for x in anchor * np.float64(rho) + (m + 0.5) * eps])))
    ids = sorted({v for v, _ in rows})
    # ---- the uploads
    Q = int(rng.choice([1, 2, 5, 17], p=[0.2, 0.3, 0.38, 0.12]))
    uploads = []
    for _ in range(Q):
        u = _upload(rng, str(rng.choice(UPLOAD_KINDS, p=UPLOAD_P / UPLOAD_P.sum())), rows, B, eps, rates, span)
        u = _specials(rng, u, 0.02 if rng.random() < 0.3 else 0.0)
        uploads.append(rng.permutation(u) if rng.random() < 0.3 else u)
    if anchor is not None:
        uploads[int(rng.integers(0, Q))] = np.concatenate([anchor, [0.0]])    # 0.0: the value the edge row is made for
    if Q == 17:                                                               # every shape beside the copies
        for i, kind in enumerate(("empty", "nan", "inf_zero", "tiny", "tiny", "tiny")):
            uploads[2 + i] = _upload(rng, kind, rows, B, eps, rates, span)
        uploads[9] = uploads[9][:1] if uploads[9].size else np.array([1.0])
    longest = max([u.size for u in uploads] + [1])
    lens = sorted({u.size for u in uploads if 0 < u.size < longest})
    # a batch whose max_query_len is below its longest upload: that upload is a refused query, not an error
    max_query_len = int(lens[-1]) if lens and rng.random() < 0.3 else int(longest)
    # ---- the steps
    gap_on = rng.random() < 0.8
    gap_first = rng.random() < 0.5
    steps = [dict(op="gap", gap_eps=gap_eps)] if gap_on and gap_first else []
    steps.append(dict(op="upload"))
    if gap_on and not gap_first:
        steps.append(dict(op="gap", gap_eps=gap_eps))
    steps += _calls(rng, int(rng.integers(3, 7)), ids, Q, gap_on)
    cheap = False
    if rng.random() < 0.4:
        if gap_on and rng.random() < 0.15:
            # enough new rows that the code table's delta fills and its index is rebuilt behind the upserts
            cheap = True
            for i in range(GAP_DELTA_ROWS + 90):
                steps.append(dict(op="upsert", id=40000 + i, keys=_cuts(rng, int(rng.integers(4, 7)), span, None), bulk=True))
        for _ in range(int(rng.choice([1, 3, 12]))):
            u = rng.random()
            vid = int(rng.choice(ids)) if u < 0.6 else int(rng.integers(5000, 5040))
            src = uploads[int(rng.integers(0, Q))]
            keys = np.zeros(0) if rng.random() < 0.12 else \
                (src[:150] + _shift(rng, B, eps, "in") if rng.random() < 0.4 and src.size else
                 _specials(rng, _cuts(rng, int(rng.choice([1, 3, 30, 120])), span, float(rng.choice(GRIDS)))))
            steps.append(dict(op="upsert", id=vid, keys=np.asarray(keys, dtype=np.float64)))
        if rng.random() < 0.3:
            steps.append(dict(op="build_index"))
        ids2 = sorted(set(ids) | {s["id"] for s in steps if s["op"] == "upsert" and not s.get("bulk")})
        steps += _calls(rng, int(rng.integers(2, 5)), ids2, Q, gap_on, cheap)
        ids = ids2
    if rng.random() < 0.25 and not cheap:
        calls = [_topk_call(rng, f, ids, Q) for f in TOPK_FORMS]
        for form in ("parts", "parts_flags"):
            k = int(rng.integers(1, max(1, 24 // Q) + 1))
            calls.append(dict(form=form, src="random", k=k, min_votes=int(rng.choice([1, 2, 5])), max_parts=int(rng.integers(1, 5)),
                              ids=[[int(rng.choice(ids + ids + [-1, 987654])) for _ in range(k)] for _ in range(Q)]))
        if gap_on:
            calls += [_cand_call(rng, "candidates", ids, Q), _cand_call(rng, "candidates_rates", ids, Q)]
        steps.append(dict(op="shards", R=int(rng.choice([1, 2, 3, 5, 8])), calls=calls))
    return dict(eps=eps, B=B, b_kind=b_kind, max_offset=max_offset, rates=rates, gap_eps=gap_eps, rows=rows,
                uploads=uploads, max_query_len=max_query_len, steps=steps)


def cases(seed, max_cases, big=False):
    rng = np.random.default_rng(seed)
    for _ in range(max_cases):
        yield gen_case(rng, big)


def case_digest(case):
    """sha256 over every byte of a case: its parameters, table, uploads and steps"""
    h = hashlib.sha256()

    def feed(x):
        if isinstance(x, np.ndarray):
            h.update(x.dtype.str.encode() + np.ascontiguousarray(x).tobytes())
        elif isinstance(x, dict):
            for k in sorted(x):
                h.update(k.encode())
                feed(x[k])
        elif isinstance(x, (list, tuple)):
            h.update(b"[%d" % len(x))
            for y in x:
                feed(y)
        elif isinstance(x, float):
            h.update(np.float64(x).tobytes())
        else:
            h.update(repr(x).encode())
    feed(case)
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------ the contract
def check_case(case):
    """Every parameter of every call of a case against the documented ranges (include/tvz.h, include/tvz_gap*.h), with
    the argument checks of the host wrappers where they exist (service.check_near, check_near_rates): raises ValueError
    for what a call would answer with an error."""
    from tvidz_amd import service
    eps, mo, rates = case["eps"], case["max_offset"], case["rates"]
    Q, L = len(case["uploads"]), case["max_query_len"]
    if not (1 <= L <= tc.ALIGN_TOPK_MAX_LEN) or any(u.ndim != 1 for u in case["uploads"]):
        raise ValueError(("max_query_len", L))
    if not (0.0 < case["gap_eps"] < math.inf):
        raise ValueError(("gap_eps", case["gap_eps"]))
    per_id = {}
    for v, _ in case["rows"]:
        per_id[v] = per_id.get(v, 0) + 1
    if any(not 0 <= v < (1 << 31) for v in per_id) or max(per_id.values()) > tc.ALIGN_PARTS_MAX_ROWS:
        raise ValueError("ids")

    def topk(p):
        f = TOPK_FORMS[p["form"]]
        service.check_near(f, eps, bounded_offset(case) if p["form"] == "topk" else mo, p["k"], p["min_votes"], p["min_score"],
                           p["contain"], p["local"], p["two_bins"])
        if (p["contain"] and "contain" not in f.flags) or (p["local"] and "local" not in f.flags):
            raise ValueError(("flags", p))
        if f.rates:
            service.check_near_rates(rates)
        excl(p)

    def excl(p):
        if p["exclude_ids"] is not None and len(p["exclude_ids"]) != Q:
            raise ValueError(("exclude_ids", p))

    def cand(p):
        if not (1 <= p["c"] <= tc.ALIGN_CANDIDATES_MAX_C and p["cap"] >= p["c"] and p["min_count"] >= 1):
            raise ValueError(("candidates", p))
        if p["form"] == "candidates_rates":
            service.check_near_rates(rates)
            if Q * len(rates) > 65535:
                raise ValueError("Q * n_rates")
        excl(p)

    def parts(p):
        service.check_near(tc.FORM_SPAN, eps, mo, p["k"], p["min_votes"], 0)
        service.check_near_rates(rates)
        if not 1 <= p["max_parts"] <= tc.ALIGN_MAX_PARTS:
            raise ValueError(("max_parts", p))
        if "span" in p:
            topk(p["span"])
        if "cand" in p:
            cand(p["cand"])
        if "ids" in p and (len(p["ids"]) != Q or any(len(r) != p["k"] for r in p["ids"])):
            raise ValueError(("ids", p))

    gap = False
    for s in case["steps"]:
        if s["op"] == "gap":
            gap = s["gap_eps"] > 0
        for p in ([s] if s["op"] == "call" else s["calls"] if s["op"] == "shards" else []):
            if p["form"] in TOPK_FORMS:
                topk(p)
            elif p["form"] in ("parts", "parts_flags"):
                parts(p)
                if "cand" in p and not gap:
                    raise ValueError("candidates without gap codes")
            else:
                cand(p)
                if not gap:
                    raise ValueError("candidates without gap codes")
        if s["op"] == "shards" and not 1 <= s["R"] <= 16:
            raise ValueError(("R", s["R"]))
        if s["op"] == "upsert" and not 0 <= s["id"] < (1 << 31):
            raise ValueError(("id", s["id"]))


def bounded_offset(case):
    """max_offset of the bounded call of a case: the case's range, cut to the 4,095 bins tvz_align_topk takes"""
    return offset_for(min(case["B"], ONE_WINDOW_B), case["eps"])


# ------------------------------------------------------------------------------------------- the expected answers
def apply_upsert(rows, v, ts):
    """db.py's add_timestamps: the FIRST row of the id is replaced, a new id is appended (fuzz_cases.apply_upsert)"""
    first = next((i for i, (vv, _) in enumerate(rows) if vv == v), None)
    if first is None:
        rows.append((v, ts))
    else:
        rows[first] = (v, ts)


def form_name(p):
    """the counter a call is counted under"""
    f = p["form"]
    if f == "wide":
        return "wide_two_bins" if p["two_bins"] else "wide_contain" if p["contain"] else "wide"
    if f == "span":
        return "span_local" if p["local"] else "span"
    return f


class Expect:
    """The table as the host sees it and the expected blocks of the calls, from `refs`."""

    def __init__(self, case, refs=REFS, stats=None):
        self.case, self.refs = case, refs
        self.rows = []
        self.queries = [u.tolist() for u in case["uploads"]]
        self.L = case["max_query_len"]
        self.live = [i for i, q in enumerate(self.queries) if len(q) <= self.L]
        self.mo = tc.ALIGN_WIDE_MAX_B * case["eps"] if case["max_offset"] is None else case["max_offset"]
        self.mo_b = bounded_offset(case)
        self.stats = stats if stats is not None else new_stats()
        self.memo = {}

    # -- the table
    def upload(self):
        self.rows = [(v, k.tolist()) for v, k in self.case["rows"]]
        self.memo.clear()

    def upsert(self, v, keys):
        apply_upsert(self.rows, v, keys.tolist())
        self.memo.clear()

    # -- the votes of every (upload, row) pair, once per state of the table
    def aligned(self, kind, rates=None):
        key = (kind, tuple(rates) if rates is not None else None)
        if key not in self.memo:
            eps, r = self.case["eps"], self.refs
            one = {"topk": lambda q: r.align(self.rows, q, eps, self.mo_b),
                   "wide": lambda q: r.wide(self.rows, q, eps, self.mo),
                   "rates": lambda q: r.rates(self.rows, q, eps, self.mo, list(rates)),
                   "span": lambda q: r.span(self.rows, q, eps, self.mo, list(rates)),
                   "two_bins": lambda q: r.two_bins(self.rows, q, eps, self.mo, list(rates))}[kind]
            self.memo[key] = [one(q) if i in self.live else None for i, q in enumerate(self.queries)]
            self.count_votes(kind, rates, self.memo[key])
        return self.memo[key]

    def topk(self, p):
        c, f = self.case, p["form"]
        common = dict(min_votes=p["min_votes"], min_score=p["min_score"], exclude_ids=p["exclude_ids"], max_query_len=self.L)
        rates = c["rates"] if TOPK_FORMS[f].rates else [1.0]
        if p["two_bins"]:
            out = atb.topk_two_bins_ref(f, self.rows, self.queries, c["eps"], self.mo, p["k"], rates=rates, contain=p["contain"],
                                        local=p["local"], aligned=self.aligned("two_bins", rates), **common)
        elif f == "topk":
            out = atr.topk_ref(self.rows, self.queries, c["eps"], self.mo_b, p["k"], aligned=self.aligned("topk"), **common)
        elif f == "wide":
            out = awr.topk_wide_ref(self.rows, self.queries, c["eps"], self.mo, p["k"], contain=p["contain"],
                                    aligned=self.aligned("wide"), **common)
        elif f == "rates":
            out = arr.topk_rates_ref(self.rows, self.queries, c["eps"], self.mo, rates, p["k"], contain=p["contain"],
                                     aligned=self.aligned("rates", rates), **common)
        else:
            out = asr.topk_span_ref(self.rows, self.queries, c["eps"], self.mo, rates, p["k"], contain=p["contain"],
                                    local=p["local"], aligned=self.aligned("span", rates), **common)
        t = out[:, p["k"], 1]
        self.stats["full_blocks"] += int((t > p["k"]).sum())
        self.stats["refused_queries"] += int((t == REFUSED).sum())
        if f != "topk" and c["B"] > ONE_WINDOW_B:
            self.stats["multi_window_calls"] += 1
            self.count_long_rows()
        return out

    def candidates(self, p, rows=None):
        c = self.case
        kw = dict(min_count=p["min_count"], cap=p["cap"], exclude_ids=p["exclude_ids"], max_query_len=self.L)
        rows = self.rows if rows is None else rows
        if p["form"] == "candidates":
            return self.refs.candidates(rows, self.queries, c["gap_eps"], p["c"], **kw).astype(np.int64)
        return self.refs.candidates_rates(rows, self.queries, c["gap_eps"], c["rates"], p["c"], **kw).astype(np.int64)

    def parts(self, p, ids):
        c = self.case
        if c["B"] > ONE_WINDOW_B:
            self.stats["multi_window_calls"] += 1
        kw = dict(min_votes=p["min_votes"], max_parts=p["max_parts"], max_query_len=self.L)
        if p["form"] == "parts":
            out = self.refs.parts(self.rows, self.queries, ids, c["eps"], self.mo, c["rates"], **kw)
        else:
            out = self.refs.parts_flags(self.rows, self.queries, ids, c["eps"], self.mo, c["rates"], flags=apf.TWO_BINS, **kw)
        n_parts, n_rows = out[:, :, 0, 3], out[:, :, 0, 4]
        self.stats["multi_part_pairs"] += int((n_parts >= 2).sum())
        self.stats["ids_with_several_rows"] += int(((n_rows >= 2) & (n_parts != REFUSED)).sum())
        self.stats["refused_queries"] += int((n_parts == REFUSED).any(axis=1).sum())
        return out

    def expect(self, p):
        """-> the expected blocks of one call, by name: "block"; a parts call also has "ids" and the block its ids are
        taken from ("span" / "cand")"""
        f = p["form"]
        if f in TOPK_FORMS:
            return dict(block=self.topk(p))
        if f in ("candidates", "candidates_rates"):
            out = self.candidates(p)
            t = out[:, p["c"], 1]
            self.stats["truncated_candidates"] += int(((t < 0) & (t != REFUSED)).sum())
            self.stats["refused_queries"] += int((t == REFUSED).sum())
            return dict(block=out)
        exp = {}
        if p["src"] == "span":
            exp["span"] = self.topk(p["span"])
            ids = exp["span"][:, :p["span"]["k"]:p["step"], 0][:, :p["k"]]
        elif p["src"] == "candidates":
            exp["cand"] = self.candidates(p["cand"])
            ids = exp["cand"][:, :p["cand"]["c"]:p["step"], 0][:, :p["k"]]
        else:
            ids = np.asarray(p["ids"], dtype=np.int64).reshape(len(self.queries), p["k"])
        exp["ids"] = np.ascontiguousarray(ids)
        exp["block"] = self.parts(p, exp["ids"])
        return exp

    # -- the counters that look at the votes
    def count_votes(self, kind, rates, aligned):
        c, st = self.case, self.stats
        B = c["B"]
        if kind == "two_bins" and B > ONE_WINDOW_B:
            for a in aligned:
                if a is not None:
                    st["two_bin_straddles_window"] += int(((a[:, 3] > 0) & ((a[:, 2] + B) % WINDOW == WINDOW - 1)).sum())
        live = [self.queries[i] for i in self.live][:2]
        if kind == "wide":
            # a row whose two best bins hold equally many votes (the first uploads, tables of up to 40 rows)
            for q in live:
                s = asr.sorted_query(q)
                for _, keys in self.rows[:40]:
                    _, b, ok = atb.bins_of(keys, s, c["eps"], B)
                    if ok.any():
                        h = np.sort(np.unique(b[ok], return_counts=True)[1])
                        st["best_bin_ties"] += int(h.size >= 2 and h[-1] == h[-2])
        if kind == "rates" and len(rates) > 1:
            # two rates that reach the same best votes
            for q in live:
                with np.errstate(over="ignore", invalid="ignore"):
                    v = np.stack([awr.align_wide_ref(self.rows, np.asarray(q, dtype=np.float64) * np.float64(rho), c["eps"],
                                                     self.mo)[:, 3] for rho in rates])
                best = v.max(0)
                st["rate_ties"] += int(((v == best).sum(0) >= 2)[best > 0].sum())

    def count_long_rows(self):
        """rows of more than 512 keys whose vote range [bin(c_min, x_max), bin(c_max, x_min)], clipped to [-B, B], spans
        at least two windows of the walk"""
        c = self.case
        B, eps = c["B"], c["eps"]
        for _, keys in self.rows:
            k = ar.row_set(keys)
            if k.size <= RESUME_KEYS:
                continue
            k = k[np.isfinite(k)]
            for i in self.live:
                s = asr.sorted_query(self.queries[i])
                s = s[np.isfinite(s)]
                if k.size and s.size:
                    lo = max(-B, math.floor((k[0] - s[-1]) / eps + 0.5))
                    hi = min(B, math.floor((k[-1] - s[0]) / eps + 0.5))
                    self.stats["long_row_multi_window"] += int(lo <= hi and (hi + B) // WINDOW > (lo + B) // WINDOW)


def new_stats():
    st = {k: 0 for k in ("cases", "multi_window_calls", "long_row_multi_window", "two_bin_straddles_window", "best_bin_ties",
                         "rate_ties", "full_blocks", "truncated_candidates", "refused_queries", "special_value_uploads",
                         "multi_part_pairs", "ids_with_several_rows", "upserts", "gap_rebuilds", "sharded_cases")}
    st["calls"] = {f: 0 for f in FORMS}
    return st


def add_stats(total, st):
    for k, v in st.items():
        if isinstance(v, dict):
            add_stats(total.setdefault(k, {}), v)
        else:
            total[k] = total.get(k, 0) + v
    return total


def is_special(u):
    u = np.asarray(u, dtype=np.float64)
    return bool((~np.isfinite(u) | ((u == 0.0) & np.signbit(u)) | (u == 5e-324) | (u == 1e300)).any())


def walk(seed, max_cases, refs=REFS, big=False, stats=None, only=None, device=None):
    """Generator + references: yields (case index, step index, call, expected blocks) for every call of every case, in
    order.  `only`: the forms to compute, the others are skipped.  `device`: a _Device that mirrors every step and
    makes every call (run())."""
    stats = stats if stats is not None else new_stats()
    for ci, case in enumerate(cases(seed, max_cases, big)):
        ex = Expect(case, refs, stats)
        stats["cases"] += 1
        stats["special_value_uploads"] += sum(is_special(u) for u in case["uploads"])
        gap_upserts = 0
        gap = False
        if device is not None:
            device.begin(case)
        for si, s in enumerate(case["steps"]):
            op = s["op"]
            if op == "call":
                if only is not None and s["form"] not in only:
                    continue
                stats["calls"][form_name(s)] += 1
                exp = ex.expect(s)
                if device is not None:
                    device.call(ex, s, exp, dict(seed=seed, case=ci, call=si))
                yield ci, si, s, exp
                continue
            if op == "upload":
                ex.upload()
            elif op == "upsert":
                ex.upsert(s["id"], s["keys"])
                stats["upserts"] += 1
                gap_upserts += int(gap and bool(s.get("bulk")))
                if gap_upserts == GAP_DELTA_ROWS + 1:
                    stats["gap_rebuilds"] += 1
            elif op == "gap":
                gap = True
            elif op == "shards":
                stats["sharded_cases"] += 1
                stats["calls"]["shards"] += len(s["calls"])
                stats["calls"]["merges"] += len(s["calls"])
            if device is not None:
                device.step(ex, s, dict(seed=seed, case=ci, call=si))
        if device is not None:
            device.end()


# -------------------------------------------------------------------------------------------------- on the device
def _fail(where, what, got, exp, **more):
    got, exp = np.asarray(got).astype(np.int64), np.asarray(exp).astype(np.int64)
    assert got.shape == exp.shape, ("NEAR MISMATCH", dict(where, what=what, got=got.shape, exp=exp.shape, **more))
    if np.array_equal(got, exp):
        return
    qi = int(np.argwhere((got != exp).reshape(got.shape[0], -1).any(1))[0, 0])
    raise AssertionError(("NEAR MISMATCH", dict(where, what=what, qi=qi, got=got[qi].tolist(), exp=exp[qi].tolist(), **more)))


class _Device:
    """One DeviceCorpus that mirrors the steps of the cases and makes their calls."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.dev = torch.device(device)
        self.dc = tc.DeviceCorpus(self.dev.index or 0)

    def close(self):
        self.dc.close()

    def ws(self, n):
        return self.torch.empty(max(int(n), 256), dtype=self.torch.uint8, device=self.dev)

    def begin(self, case):
        self.case = case
        self.dc.set_gap_index(0.0)
        self.dc.clear()
        self.d_q, self.d_off, _ = tc.pack_queries(case["uploads"], self.dev)
        self.Q, self.L, self.nk = len(case["uploads"]), case["max_query_len"], self.d_q.numel()
        self.gap_builds = None

    def end(self):
        pass

    def step(self, ex, s, where):
        op = s["op"]
        if op == "gap":
            self.dc.set_gap_index(s["gap_eps"])
        elif op == "upload":
            self.dc.upload(ex.rows)
        elif op == "upsert":
            if s.get("bulk") and self.gap_builds is None:
                self.gap_builds = self.dc.gap_index_stats()["builds"]
            self.dc.upsert(s["id"], s["keys"])
            if s.get("bulk") and s["id"] == 40000 + GAP_DELTA_ROWS + 89:
                # the rebuild runs in the upserting thread: it is over when the last upsert has returned
                st = self.dc.gap_index_stats()
                assert st["builds"] > self.gap_builds and st["rows"] == len(ex.rows), ("NO GAP REBUILD", dict(where, stats=st))
        elif op == "build_index":
            self.dc.build_index()
        elif op == "shards":
            self.shards(ex, s, where)

    # -- the single calls
    def excl(self, p):
        if p.get("exclude_ids") is None:
            return None
        return self.torch.tensor(p["exclude_ids"], dtype=self.torch.int32, device=self.dev)

    def ask(self, p, **over):
        """the keywords of a top-k form's block call"""
        c, f = self.case, TOPK_FORMS[p["form"]]
        a = dict(eps=c["eps"], max_offset=bounded_offset(c) if p["form"] == "topk" else c["max_offset"], min_votes=p["min_votes"],
                 min_score=p["min_score"])
        if f.rates:
            a["rates"] = c["rates"]
        if f.flags:
            a["contain"], a["two_bins"] = p["contain"], p["two_bins"]
        if "local" in f.flags:
            a["local"] = p["local"]
        a.update(over)
        return a

    def topk_block(self, dc, form, p, **over):
        f = TOPK_FORMS[form]
        ws = self.ws(tc.form_workspace_bytes(f, self.Q, self.L, self.nk, p["k"]))
        return getattr(dc, f.stem + "_block")(self.d_q, self.d_off, self.L, k=p["k"], d_exclude_ids=self.excl(p), workspace=ws,
                                              **self.ask(dict(p, form=form), **over))

    def cand_block(self, dc, p, rates=None):
        kw = dict(c=p["c"], min_count=p["min_count"], cap=p["cap"], d_exclude_ids=self.excl(p))
        if p["form"] == "candidates" and rates is None:
            ws = self.ws(tc.align_candidates_workspace_bytes(self.Q, self.L, self.nk, p["cap"], p["c"]))
            return dc.align_candidates_block(self.d_q, self.d_off, self.L, workspace=ws, **kw)
        rates = self.case["rates"] if rates is None else rates
        ws = self.ws(tc.align_candidates_rates_workspace_bytes(self.Q, self.L, self.nk, len(rates), p["cap"], p["c"]))
        return dc.align_candidates_rates_block(self.d_q, self.d_off, self.L, rates, workspace=ws, **kw)

    def parts_kw(self, p):
        c = self.case
        return dict(eps=c["eps"], max_offset=c["max_offset"], rates=c["rates"], min_votes=p["min_votes"], max_parts=p["max_parts"],
                    two_bins=p["form"] == "parts_flags")

    def parts_block(self, dc, p, d_ids):
        ws = self.ws(tc.align_parts_workspace_bytes(self.Q, self.L, self.nk, d_ids.shape[1], p["max_parts"]))
        return dc.align_parts_block(self.d_q, self.d_off, self.L, d_ids, workspace=ws, **self.parts_kw(p))

    def ids_tensor(self, ids, transposed=False):
        t = self.torch.from_numpy(np.ascontiguousarray(np.asarray(ids, dtype=np.int32)))
        return t.t().contiguous().to(self.dev).t() if transposed else t.to(self.dev)

    def call(self, ex, p, exp, where):
        f = p["form"]
        where = dict(where, form=form_name(p))
        if f in TOPK_FORMS:
            got = self.topk_block(self.dc, f, p)
            _fail(where, "block", got.cpu().numpy(), exp["block"])
            self.relations(p, got, where)
        elif f in ("candidates", "candidates_rates"):
            got = self.cand_block(self.dc, p).cpu().numpy()
            self.check_candidates(where, "block", got, exp["block"], p["c"])
            ids = [v for v, _ in ex.rows]
            if f == "candidates" and len(set(ids)) == len(ids):
                # over distinct ids, the call with the single rate 1.0 names the same ids with the same counts
                one = self.cand_block(self.dc, dict(p, form="candidates_rates"), rates=(1.0,)).cpu().numpy()
                exact = exp["block"][:, p["c"], 1] >= 0
                _fail(where, "candidates_rates (1.0,) == candidates", one[exact][:, :, :2], got[exact])
        else:
            if p["src"] == "span":
                src = self.topk_block(self.dc, "span", p["span"])
                _fail(where, "the span block the ids come from", src.cpu().numpy(), exp["span"])
                d_ids = src[:, :p["span"]["k"]:p["step"], 0][:, :p["k"]]
            elif p["src"] == "candidates":
                src = self.cand_block(self.dc, p["cand"])
                exact = self.check_candidates(where, "the candidates block the ids come from", src.cpu().numpy(), exp["cand"],
                                              p["cand"]["c"])
                if not exact:                    # (a list beyond cap: the library's rows may differ; the reference's are passed)
                    src = self.torch.from_numpy(exp["cand"].astype(np.int32)).to(self.dev)
                d_ids = src[:, :p["cand"]["c"]:p["step"], 0][:, :p["k"]]
            else:
                d_ids = self.ids_tensor(exp["ids"], p.get("transposed", False))
            _fail(where, "ids", d_ids.cpu().numpy(), exp["ids"])
            _fail(where, "block", self.parts_block(self.dc, p, d_ids).cpu().numpy().reshape(self.Q, -1),
                  exp["block"].reshape(self.Q, -1))

    def check_candidates(self, where, what, got, exp, c):
        """whole blocks; where a total says the list went beyond cap, the totals row only (the contract's rule)"""
        exact = exp[:, c, 1] >= 0
        exact |= exp[:, c, 1] == REFUSED
        _fail(where, what + " (totals)", got[:, c], exp[:, c])
        _fail(where, what, got[exact], exp[exact])
        return bool(exact.all())

    def relations(self, p, got, where):
        """what include/tvz.h says of two forms' blocks, on the blocks of this call"""
        f = p["form"]
        if f == "topk":
            wide = self.topk_block(self.dc, "wide", dict(p, contain=False, local=False, two_bins=False),
                                   max_offset=bounded_offset(self.case))
            _fail(where, "wide == bounded for B <= 2047", wide.cpu().numpy(), got.cpu().numpy())
        elif f == "wide":
            one = self.topk_block(self.dc, "rates", p, rates=(1.0,)).cpu().numpy()
            _fail(where, "rates (1.0,) == wide, columns 0..3", one[:, :, :4], got.cpu().numpy())
            _fail(where, "rates (1.0,): rate index 0", one[:, :, 4], np.zeros_like(one[:, :, 4]))
        elif f == "rates":
            span = self.topk_block(self.dc, "span", dict(p, local=False)).cpu().numpy()
            _fail(where, "span == rates, columns 0..4", span[:, :, :5], got.cpu().numpy())

    # -- the sharded round
    def shards(self, ex, s, where):
        from tvidz_amd import service
        torch, R = self.torch, s["R"]
        sc = service.ShardedCorpus(self.dev.index or 0, n_shards=R)
        try:
            sc.upload(ex.rows)
            gap = any(p["form"].startswith("candidates") for p in s["calls"])
            if gap:
                sc.set_gap_index(self.case["gap_eps"])
            queries = (self.d_q, self.d_off)
            for n, p in enumerate(s["calls"]):
                f = p["form"]
                w = dict(where, form=form_name(p), R=R, sharded_call=n)
                if f in TOPK_FORMS:
                    one = self.topk_block(self.dc, f, p).cpu().numpy()
                    k, form = p["k"], TOPK_FORMS[f]
                    ask = self.ask(p)
                    rows, totals = getattr(sc, form.stem)(queries, k=k, exclude_ids=self.excl(p), max_query_len=self.L, **ask)
                    _fail(w, "ShardedCorpus rows == DeviceCorpus", rows, one[:, :k])
                    _fail(w, "ShardedCorpus totals == DeviceCorpus", totals, one[:, k, 1])
                    ws = self.ws(tc.form_workspace_bytes(form, self.Q, self.L, self.nk, k))
                    blocks, m_rows, m_totals = tc.form_shards(form, sc.shards, self.d_q, self.d_off, self.L, k, ws, self.excl(p),
                                                              **ask)
                    _fail(w, "_shards rows == DeviceCorpus", m_rows.cpu().numpy(), one[:, :k])
                    _fail(w, "_shards totals == DeviceCorpus", m_totals.cpu().numpy(), one[:, k, 1])
                    flags = {name: p[name] for name in form.flags}
                    d_rows, d_totals = tc.form_merge(form, blocks, k, self.d_q, self.d_off, two_bins=p["two_bins"], **flags)
                    _fail(w, "device merge rows == _shards", d_rows.cpu().numpy(), m_rows.cpu().numpy())
                    _fail(w, "device merge totals == _shards", d_totals.cpu().numpy(), m_totals.cpu().numpy())
                    if f in ("rates", "span"):
                        ref = arr.merge_ref if f == "rates" else asr.merge_ref
                        h_rows, h_totals = ref(blocks.cpu().numpy(), ex.queries, **flags)
                        _fail(w, "device merge rows == merge_ref", d_rows.cpu().numpy(), h_rows)
                        _fail(w, "device merge totals == merge_ref", d_totals.cpu().numpy(), h_totals)
                elif f in ("parts", "parts_flags"):
                    d_ids = self.ids_tensor(p["ids"])
                    one = self.parts_block(self.dc, p, d_ids).cpu().numpy()
                    got = sc.align_parts(queries, d_ids, max_query_len=self.L, **self.parts_kw(p))
                    _fail(w, "ShardedCorpus parts == DeviceCorpus", got.reshape(self.Q, -1), one.reshape(self.Q, -1))
                    ws = self.ws(tc.align_parts_workspace_bytes(self.Q, self.L, self.nk, p["k"], p["max_parts"]))
                    blocks, merged = tc.align_parts_shards(sc.shards, self.d_q, self.d_off, self.L, d_ids, workspace=ws,
                                                           **self.parts_kw(p))
                    host = tc.align_parts_merge(blocks.cpu().numpy())
                    _fail(w, "_shards parts == host merge", merged.cpu().numpy().reshape(self.Q, -1), host.reshape(self.Q, -1))
                    _fail(w, "device merge parts == host merge", tc.align_parts_merge_device(blocks).cpu().numpy().reshape(self.Q, -1),
                          host.reshape(self.Q, -1))
                    _fail(w, "_shards parts == DeviceCorpus", merged.cpu().numpy().reshape(self.Q, -1), one.reshape(self.Q, -1))
                else:
                    one = self.cand_block(self.dc, p).cpu().numpy()
                    kw = dict(c=p["c"], min_count=p["min_count"], cap=p["cap"])
                    if f == "candidates":
                        ws = self.ws(tc.align_candidates_workspace_bytes(self.Q, self.L, self.nk, p["cap"], p["c"]))
                        blocks, merged = tc.align_candidates_shards(sc.shards, self.d_q, self.d_off, self.L, d_exclude_ids=self.excl(p),
                                                                    workspace=ws, **kw)
                        host, dev_merge = tc.align_candidates_merge, tc.align_candidates_merge_device
                        got = sc.align_candidates_block(queries, exclude_ids=self.excl(p), max_query_len=self.L, **kw)
                    else:
                        rates = self.case["rates"]
                        ws = self.ws(tc.align_candidates_rates_workspace_bytes(self.Q, self.L, self.nk, len(rates), p["cap"], p["c"]))
                        blocks, merged = tc.align_candidates_rates_shards(sc.shards, self.d_q, self.d_off, self.L, rates,
                                                                          d_exclude_ids=self.excl(p), workspace=ws, **kw)
                        host, dev_merge = tc.align_candidates_rates_merge, tc.align_candidates_rates_merge_device
                        got = sc.align_candidates_rates_block(queries, rates, exclude_ids=self.excl(p), max_query_len=self.L, **kw)
                    h = host(blocks.cpu().numpy())
                    _fail(w, "_shards candidates == host merge", merged.cpu().numpy(), h)
                    _fail(w, "device merge candidates == host merge", dev_merge(blocks).cpu().numpy(), h)
                    _fail(w, "ShardedCorpus candidates == _shards", got.cpu().numpy(), merged.cpu().numpy())
                    # the whole table's answer where no shard's list went beyond cap, by the per-shard reference: the
                    # reference without a cap; and the one handle's block where ITS list did not go beyond cap either
                    fits = np.ones(self.Q, dtype=bool)
                    for r in range(R):
                        mine = [(v, k) for v, k in ex.rows if v % R == r]
                        t = ex.candidates(p, mine)[:, p["c"], 1]
                        fits &= (t >= 0) | (t == REFUSED)
                    _fail(w, "_shards candidates == the reference without a cap", merged.cpu().numpy()[fits],
                          ex.candidates(dict(p, cap=1 << 30))[fits])
                    t = ex.candidates(p)[:, p["c"], 1]
                    fits &= (t >= 0) | (t == REFUSED)
                    _fail(w, "ShardedCorpus candidates == DeviceCorpus", merged.cpu().numpy()[fits], one[fits])
            torch.cuda.synchronize(self.dev)
        finally:
            sc.close()


def run(seed, max_cases, device="cuda:0", refs=REFS, big=False, seconds=None, progress=False):
    """`max_cases` cases of `seed` (or, with `seconds`, cases until that time has passed - the soak; the slice in the
    suite is bounded by its case count alone) -> counters.  device=None: the generator and the references alone."""
    stats = new_stats()
    dev = _Device(device) if device is not None else None
    t0 = time.time()
    t_note = t0 + 30
    try:
        for _ in walk(seed, max_cases, refs, big, stats, device=dev):
            if seconds is not None and time.time() - t0 > seconds:
                break
            if progress and time.time() > t_note:
                print(json.dumps({"progress": stats}), flush=True)
                t_note = time.time() + 30
    finally:
        if dev is not None:
            dev.close()
    stats["seconds"] = round(time.time() - t0, 2)
    return stats
