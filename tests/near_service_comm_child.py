"""Child process of tests/test_near_service_gpu.py: creates the libtvz RCCL communicator BEFORE its first GPU call (as
tests/near_comm_child.py does), then runs at world size 1
  - tvz_align_rates_topk_sharded, tvz_align_span_topk_sharded and tvz_align_parts_sharded against their unsharded calls on
    the same handle, through corpus.Comm and through sharded.RcclShardedMatcher (every side stream), with their
    workspaces' bounds and the refusals that come behind the unsharded call's;
  - the Inspector with near_rates, near_score="local" and near_parts=2 over a one-rank service.RankCorpus(RcclShardedMatcher)
    against the same driver over a plain DeviceCorpus,
and prints the results as JSON."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (import only: no GPU call yet)

from tests import align_parts_cases as cs, align_span_ref as asr  # noqa: E402
from tvidz_amd import corpus as tc, sharded  # noqa: E402

comm = tc.Comm(tc.Comm.unique_id(), 1, 0, 0)           # ncclCommInitRank: the first GPU call of this process
dev = torch.device("cuda:0")
EPS = cs.EPS
L = 129
rows, uploads = cs.table(), cs.uploads()
batch = [uploads[n] for n in ("inserted", "parts24", "fps_inserted", "special", "unrelated")] + [[float(i) for i in range(150)]]
assert max(len(q) for q in batch[:-1]) == L                                    # the last one is over-long at max_query_len = L
dc = tc.DeviceCorpus(0)
dc.upload(rows)
d_q, d_off, _ = tc.pack_queries(batch, dev)
Q = len(batch)
lib = comm.lib
out = {"equal": {}, "premise": {}}
excl = [cs.FILM, -1, -1, -1, -1, -1]
d_ex = torch.tensor(excl, dtype=torch.int32, device=dev)
err = lambda: (lib.tvz_last_error() or b"").decode()                            # noqa: E731


def same(a, b):
    return bool(torch.equal(torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b))))


# ---- 1. each sharded call equals its unsharded call bit for bit ------------------------------------------------------
for k in (1, 5, 64):
    for rates in ((1.0,), (1.0, 0.96)):
        one = dc.align_rates_topk(batch, eps=EPS, rates=rates, k=k, max_query_len=L)
        r, t = comm.align_rates_topk_sharded(dc, d_q, d_off, L, eps=EPS, rates=rates, k=k)
        torch.cuda.synchronize()
        out["equal"][f"rates k={k} {rates}"] = same(r.cpu(), one[0]) and same(t.cpu(), one[1]) and tuple(r.shape) == (Q, k, 5)
        for name, kw, dkw in (("plain", {}, {}), ("local", dict(local=True, min_votes=4), dict(local=True, min_votes=4)),
                              ("contain", dict(contain=True), dict(contain=True)),
                              ("local excluded", dict(local=True, min_votes=4, exclude_ids=excl),
                               dict(local=True, min_votes=4, d_exclude_ids=d_ex))):
            one = dc.align_span_topk(batch, eps=EPS, rates=rates, k=k, max_query_len=L, **kw)
            r, t = comm.align_span_topk_sharded(dc, d_q, d_off, L, eps=EPS, rates=rates, k=k, **dkw)
            torch.cuda.synchronize()
            out["equal"][f"span {name} k={k} {rates}"] = same(r.cpu(), one[0]) and same(t.cpu(), one[1]) \
                and tuple(r.shape) == (Q, k, 8)
            if k == 5 and rates == (1.0, 0.96):
                out["premise"][name] = {"totals": one[1].tolist(), "first_ids": one[0][:, 0, 0].tolist()}
        # the parts call on the ids of the span block the search just wrote, by its strides
        block = dc.align_span_topk_block(d_q, d_off, L, eps=EPS, rates=rates, k=k, min_votes=1)
        ids = block[:, :k, 0]
        for P in (1, 4):
            one = dc.align_parts_block(d_q, d_off, L, ids, eps=EPS, rates=rates, min_votes=1, max_parts=P)
            got = comm.align_parts_sharded(dc, d_q, d_off, L, ids, eps=EPS, rates=rates, min_votes=1, max_parts=P)
            torch.cuda.synchronize()
            out["equal"][f"parts k={k} P={P} {rates}"] = same(got.cpu(), one.cpu()) and tuple(got.shape) == (Q, k, 1 + P, 6)
named = torch.tensor([list(cs.IDS)] * Q, dtype=torch.int32, device=dev)
want_parts = dc.align_parts_block(d_q, d_off, L, named, eps=EPS, rates=(1.0, 0.96), min_votes=1, max_parts=3).cpu()
got = comm.align_parts_sharded(dc, d_q, d_off, L, named, eps=EPS, rates=(1.0, 0.96), min_votes=1, max_parts=3)
torch.cuda.synchronize()
out["equal"]["parts named ids"] = same(got.cpu(), want_parts)
out["premise"]["parts"] = {"n_parts": want_parts[:, :, 0, 3].tolist(), "n_rows": want_parts[:, :, 0, 4].tolist()}

# ---- 2. the matcher: every side stream in turn ------------------------------------------------------------------------
sm = sharded.RcclShardedMatcher(dc, comm, k=16, cap=64)
out["matcher_forms"] = [f.stem for f in sm.align_forms]
out["matcher_supports"] = [sm.supports_align_rates, sm.supports_align_span, sm.supports_align_parts]
want_r = dc.align_rates_topk(batch, eps=EPS, rates=(1.0, 0.96), k=5, max_query_len=L)
want_s = dc.align_span_topk(batch, eps=EPS, rates=(1.0, 0.96), k=5, local=True, min_votes=4, max_query_len=L)
slots = []
for _ in range(3):
    r, t = sm.align_rates_topk(d_q, d_off, L, eps=EPS, rates=(1.0, 0.96), k=5)
    torch.cuda.synchronize()
    ok = same(r.cpu(), want_r[0]) and same(t.cpu(), want_r[1])
    r, t = sm.align_span_topk(d_q, d_off, L, eps=EPS, rates=(1.0, 0.96), k=5, local=True, min_votes=4)
    torch.cuda.synchronize()
    ok = ok and same(r.cpu(), want_s[0]) and same(t.cpu(), want_s[1])
    p = sm.parts(d_q, d_off, L, named, eps=EPS, rates=(1.0, 0.96), min_votes=1, max_parts=3)
    torch.cuda.synchronize()
    slots.append(ok and same(p.cpu(), want_parts))
out["matcher_slots_equal"] = slots

# ---- 3. the workspaces: exactly the sharded sizing function's bytes inside a poisoned buffer; one byte less; refusals ----
RATES2 = (C.c_double * 2)(1.0, 0.96)
stream = lambda: torch.cuda.current_stream().cuda_stream                        # noqa: E731
WIDEST = tc.ALIGN_WIDE_MAX_B * EPS


def raw_form(stem, cols, comm_h, ws_ptr, ws_bytes, rows_t, totals_t, rates=RATES2, n_rates=2, flags=0, k=5):
    return getattr(lib, f"tvz_{stem}_sharded")(dc._h, comm_h, d_q.data_ptr(), d_off.data_ptr(), Q, L, EPS, WIDEST, rates, n_rates, 1,
                                               0, flags, None, k, rows_t.data_ptr(), totals_t.data_ptr(), ws_ptr, ws_bytes, stream())


def raw_parts(comm_h, ws_ptr, ws_bytes, parts_t, rates=RATES2, n_rates=2, P=3):
    return lib.tvz_align_parts_sharded(dc._h, comm_h, d_q.data_ptr(), d_off.data_ptr(), Q, L, named.data_ptr(), 1, named.shape[1],
                                       named.shape[1], EPS, WIDEST, rates, n_rates, 1, P, parts_t.data_ptr(), ws_ptr, ws_bytes,
                                       stream())


SENT = -0x5A5A5A5A
bounds = {}
for stem, cols, want in (("align_rates_topk", 5, want_r), ("align_span_topk", 8, dc.align_span_topk(batch, eps=EPS, rates=(1.0, 0.96),
                                                                                                  k=5, max_query_len=L))):
    form = {5: tc.FORM_RATES, 8: tc.FORM_SPAN}[cols]
    n = tc.form_workspace_bytes(form, Q, L, d_q.numel(), 5, 1)
    least = tc.form_workspace_bytes(form, Q, L, L, 5, 1)
    res = []
    for extra in (0, 8, 248):
        buf = torch.full((4096 + 256 + n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        lo = 4096 + (-(buf.data_ptr() + 4096)) % 256 + extra
        # (guards of four queries' rows: 4 x 5 x cols x 4 bytes keep the output 16-byte aligned, which the merge asks for)
        r5 = torch.full((Q + 8, 5, cols), SENT, dtype=torch.int32, device=dev)
        t5 = torch.full((Q + 8,), SENT, dtype=torch.int32, device=dev)
        rc = raw_form(stem, cols, comm._h, buf.data_ptr() + lo, n, r5[4:Q + 4], t5[4:Q + 4])
        torch.cuda.synchronize()
        res.append(rc == 0 and bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + n:] == 0xA5).all())
                   and same(r5[4:Q + 4].cpu(), want[0]) and same(t5[4:Q + 4].cpu(), want[1])
                   and bool((r5[:4] == SENT).all()) and bool((r5[Q + 4:] == SENT).all()) and bool((t5[:4] == SENT).all())
                   and bool((t5[Q + 4:] == SENT).all()))
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    r5 = torch.full((Q, 5, cols), SENT, dtype=torch.int32, device=dev)
    t5 = torch.full((Q,), SENT, dtype=torch.int32, device=dev)
    refusals = {}
    refusals["short"] = [raw_form(stem, cols, comm._h, ws.data_ptr(), least - 1, r5, t5), err()]
    refusals["null_comm"] = [raw_form(stem, cols, None, ws.data_ptr(), n, r5, t5), err()]
    refusals["null_comm_and_no_rates"] = [raw_form(stem, cols, None, ws.data_ptr(), n, r5, t5, n_rates=0), err()]
    refusals["null_comm_and_short"] = [raw_form(stem, cols, None, ws.data_ptr(), least - 1, r5, t5), err()]
    refusals["bad_flag"] = [raw_form(stem, cols, comm._h, ws.data_ptr(), n, r5, t5, flags=4), err()]
    refusals["k65"] = [raw_form(stem, cols, comm._h, ws.data_ptr(), n, r5, t5, k=65), err()]
    torch.cuda.synchronize()
    refusals["nothing_written"] = bool((r5 == SENT).all()) and bool((t5 == SENT).all())
    refusals["least_ok"] = raw_form(stem, cols, comm._h, ws.data_ptr(), least, r5, t5)
    torch.cuda.synchronize()
    bounds[stem] = {"exact": res, "sizes": [n, least, tc.form_workspace_bytes(form, Q, L, d_q.numel(), 5)], **refusals}
k_named = named.shape[1]
n = tc.align_parts_sharded_workspace_bytes(Q, L, d_q.numel(), k_named, 3, 1)
least = tc.align_parts_sharded_workspace_bytes(Q, L, L, k_named, 3, 1)
res = []
for extra in (0, 8, 248):
    buf = torch.full((4096 + 256 + n + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    lo = 4096 + (-(buf.data_ptr() + 4096)) % 256 + extra
    p3 = torch.full((Q + 2, k_named, 4, 6), SENT, dtype=torch.int32, device=dev)
    rc = raw_parts(comm._h, buf.data_ptr() + lo, n, p3[1:Q + 1])
    torch.cuda.synchronize()
    res.append(rc == 0 and bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + n:] == 0xA5).all()) and same(p3[1:Q + 1].cpu(), want_parts)
               and bool((p3[0] == SENT).all()) and bool((p3[Q + 1] == SENT).all()))
ws = torch.empty(n, dtype=torch.uint8, device=dev)
p3 = torch.full((Q, k_named, 4, 6), SENT, dtype=torch.int32, device=dev)
refusals = {}
refusals["short"] = [raw_parts(comm._h, ws.data_ptr(), least - 1, p3), err()]
refusals["null_comm"] = [raw_parts(None, ws.data_ptr(), n, p3), err()]
refusals["null_comm_and_no_rates"] = [raw_parts(None, ws.data_ptr(), n, p3, n_rates=0), err()]
refusals["null_comm_and_short"] = [raw_parts(None, ws.data_ptr(), least - 1, p3), err()]
refusals["parts5"] = [raw_parts(comm._h, ws.data_ptr(), n, p3, P=5), err()]
torch.cuda.synchronize()
refusals["nothing_written"] = bool((p3 == SENT).all())
refusals["least_ok"] = raw_parts(comm._h, ws.data_ptr(), least, p3)
torch.cuda.synchronize()
bounds["align_parts"] = {"exact": res, "sizes": [n, least, tc.align_parts_workspace_bytes(Q, L, d_q.numel(), k_named, 3)], **refusals}
out["bounds"] = bounds
dc.close()

# ---- 4. the driver: Inspector._near over a plain DeviceCorpus and over a one-rank RankCorpus --------------------------
from tvidz_amd import inspector as insp, service  # noqa: E402

film24 = cs.film()
fast = [x * 24.0 / 25.0 + 12.3 for x in film24]                 # the film at 25 fps behind 12.3 s of something else
film400, compilation, clip, shift = asr.compilation_case()
COMP = 500
table = rows + [(COMP, film400)]
base = dict(device="cuda:0", near_duplicates=True, near_top_k=8, near_any_offset=True)
scenarios = {
    "fps": (fast, dict(base, near_rates=(1.0, 25.0 / 24.0))),
    "fps_unrated": (fast, dict(base)),
    "compilation_local": (compilation, dict(base, near_score="local", near_min_votes=8, near_jaccard=0.5)),
    "compilation_containment": (compilation, dict(base, near_score="containment", near_min_votes=8, near_jaccard=0.5)),
    "inserted_parts": (uploads["inserted"], dict(base, near_score="local", near_min_votes=8, near_jaccard=0.9, near_parts=2)),
}


def run(corpus):
    class Store:
        def get_video_by_id(self, vid):
            return None
    Store.corpus = corpus
    return {name: insp.Inspector(Store(), **kw)._near(424242, upload) for name, (upload, kw) in scenarios.items()}


plain = tc.DeviceCorpus(0)
plain.upload(table)
out["near_plain"] = run(plain)
plain.close()
shard = tc.DeviceCorpus(0)
rc = service.RankCorpus(shard, sharded.RcclShardedMatcher(shard, comm, k=8, cap=64), xdev="cpu")
rc.upload(table)
out["rank_supports"] = [rc.supports_align_wide, rc.supports_align_rates, rc.supports_align_span, rc.supports_align_parts]
out["near_rank"] = run(rc)
# what the caller refuses never reaches the tick; an over-long query is answered without travelling
ticks = rc.busy_ticks
refused = []
for call in (lambda: rc.align_rates_topk([[1.0, 2.0]], eps=EPS, rates=(), k=4),
             lambda: rc.align_span_topk([[1.0, 2.0]], eps=EPS, rates=(1.0, -1.0), k=4),
             lambda: rc.align_span_topk([[1.0, 2.0]], eps=EPS, k=4, contain=True, local=True),
             lambda: rc.align_parts([[1.0, 2.0]], [[1]], eps=EPS, min_votes=1, max_parts=5),
             lambda: rc.align_parts([[1.0, 2.0]], [[1]], eps=EPS, min_votes=0, max_parts=2)):
    try:
        call()
        refused.append("accepted")
    except ValueError:
        refused.append("ValueError")
long_rows, long_totals = rc.align_span_topk([[0.5] * 4096], eps=EPS, k=4)
long_parts = rc.align_parts([[0.5] * 4096], [[cs.FILM, -1]], eps=EPS, min_votes=1, max_parts=2)
out["caller"] = {"refused": refused, "long_totals": long_totals.tolist(), "long_parts": long_parts.tolist(),
                 "ticks_unchanged": rc.busy_ticks == ticks}
out["rank_broken"] = repr(rc.broken) if rc.broken else None
rc.close()
comm.close()
print("RESULT " + json.dumps(out))
