"""What tests/test_py_prelude_gpu.py (the thirteen wrappers that need no communicator) and tests/comm_child.py (the three
of corpus.Comm) ask of every batched wrapper of tvidz_amd.corpus: bad queries, a workspace one byte short or a
mis-shaped output raise RuntimeError and leave outputs that were filled with a sentinel as they were, and a workspace
of exactly the sizing function's bytes is accepted.

A 4-row table, Q = 2, k = 2.  The second query is empty, so the batch's keys are one query's: the shape at which the
sizing function's answer is also the least tvz_align_topk_shards takes (that wrapper leaves the size of its workspace
to the library, which accepts one down to a single query's room and refuses the other queries one by one)."""
import torch

from tvidz_amd import corpus as tc

ROWS = [(10, [1.0, 2.5, 4.0, 7.25]), (11, [1.0, 2.5, 9.0]), (12, [20.0, 21.5]), (13, [4.0, 7.25, 30.0])]
QUERIES = [[1.0, 2.5, 4.0, 7.25], []]
Q, K, CAP, MM, TOL = 2, 2, 4, 2, 0.01
NEAR = dict(eps=0.1, max_offset=1.0, k=K)
RATES = (1.0, 25 / 24)
SENTINEL = -7
DEV = "cuda:0"
# every other refusal is Python's
LEFT_TO_THE_LIBRARY = {(name, "a workspace one byte short") for name in
                       ("align_topk_shards", "align_wide_topk_shards", "align_rates_topk_shards", "align_span_topk_shards")}


def _full(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)


def batch():
    return tc.pack_queries(QUERIES, torch.device(DEV))


def wrappers(shards, comm=None):
    """name -> (call(d_q, d_off, workspace, out), the sizing function's bytes for batch(), good(): sentinel-filled
    outputs, bad(): mis-shaped ones) of the wrappers of the handles `shards` (the single-handle ones: of the first), or
    of `comm` over the first.  The *_shards forms make their outputs themselves: good and bad are None."""
    dc = shards[0]
    _, _, L = batch()
    n = sum(len(q) for q in QUERIES)

    def hits():
        return (_full(Q, CAP, 3), _full(Q)), (_full(Q, CAP - 1, 3), _full(Q))

    def block(w):
        return _full(Q, K + 1, w), _full(Q, K, w)

    def pair(w):
        return (_full(Q, K, w), _full(Q)), (_full(Q, K + 1, w), _full(Q))

    def good_and_bad(make, *a):
        """The two factories of a spec: fresh sentinel-filled outputs of the right shape, and of a wrong one."""
        return (lambda: make(*a)[0], lambda: make(*a)[1])

    if comm is not None:
        R = comm.n_ranks
        return {
            "match_sharded": (lambda q, o, ws, out: comm.match_sharded(dc, q, o, L, MM, CAP, K, workspace=ws, out=out),
                              tc.workspace_bytes(Q, L, CAP, K, R, n)) + good_and_bad(pair, 3),
            "match_tol_sharded": (lambda q, o, ws, out: comm.match_tol_sharded(dc, q, o, L, TOL, MM, K, workspace=ws, out=out),
                                  tc.tol_topk_workspace_bytes(Q, L, n, K, R)) + good_and_bad(pair, 3),
            "align_topk_sharded": (lambda q, o, ws, out: comm.align_topk_sharded(dc, q, o, L, workspace=ws, out=out, **NEAR),
                                   tc.align_topk_sharded_workspace_bytes(Q, L, n, K, R)) + good_and_bad(pair, 4),
        }
    return {
        "match": (lambda q, o, ws, out: dc.match(q, o, L, MM, CAP, out_hits=out[0], out_n=out[1], workspace=ws),
                  tc.workspace_bytes(Q, L, total_query_keys=n)) + good_and_bad(hits),
        "match_tol": (lambda q, o, ws, out: dc.match_tol(q, o, L, TOL, MM, CAP, out_hits=out[0], out_n=out[1], workspace=ws),
                      tc.tol_workspace_bytes(Q, L, n)) + good_and_bad(hits),
        "match_topk": (lambda q, o, ws, out: dc.match_topk(q, o, L, MM, CAP, K, out=out, workspace=ws),
                       tc.workspace_bytes(Q, L, CAP, K, total_query_keys=n)) + good_and_bad(block, 3),
        "match_tol_topk": (lambda q, o, ws, out: dc.match_tol_topk(q, o, L, TOL, MM, K, out=out, workspace=ws),
                           tc.tol_topk_workspace_bytes(Q, L, n, K)) + good_and_bad(block, 3),
        "align_topk_block": (lambda q, o, ws, out: dc.align_topk_block(q, o, L, out=out, workspace=ws, **NEAR),
                             tc.align_topk_workspace_bytes(Q, L, n, K)) + good_and_bad(block, 4),
        "match_topk_shards": (lambda q, o, ws, out: tc.match_topk_shards(shards, q, o, L, MM, CAP, K, ws),
                              tc.workspace_bytes(Q, L, CAP, K, total_query_keys=n), None, None),
        "align_topk_shards": (lambda q, o, ws, out: tc.align_topk_shards(shards, q, o, L, workspace=ws, **NEAR),
                              tc.align_topk_workspace_bytes(Q, L, n, K), None, None),
        "align_wide_topk_block": (lambda q, o, ws, out: dc.align_wide_topk_block(q, o, L, out=out, workspace=ws, **NEAR),
                                  tc.align_wide_topk_workspace_bytes(Q, L, n, K)) + good_and_bad(block, 4),
        "align_rates_topk_block": (lambda q, o, ws, out: dc.align_rates_topk_block(q, o, L, rates=RATES, out=out,
                                                                                   workspace=ws, **NEAR),
                                   tc.align_rates_topk_workspace_bytes(Q, L, n, K)) + good_and_bad(block, 5),
        "align_span_topk_block": (lambda q, o, ws, out: dc.align_span_topk_block(q, o, L, rates=RATES, out=out,
                                                                                 workspace=ws, **NEAR),
                                  tc.align_span_topk_workspace_bytes(Q, L, n, K)) + good_and_bad(block, 8),
        "align_wide_topk_shards": (lambda q, o, ws, out: tc.align_wide_topk_shards(shards, q, o, L, workspace=ws, **NEAR),
                                   tc.align_wide_topk_workspace_bytes(Q, L, n, K), None, None),
        "align_rates_topk_shards": (lambda q, o, ws, out: tc.align_rates_topk_shards(shards, q, o, L, rates=RATES,
                                                                                     workspace=ws, **NEAR),
                                    tc.align_rates_topk_workspace_bytes(Q, L, n, K), None, None),
        "align_span_topk_shards": (lambda q, o, ws, out: tc.align_span_topk_shards(shards, q, o, L, rates=RATES,
                                                                                   workspace=ws, **NEAR),
                                   tc.align_span_topk_workspace_bytes(Q, L, n, K), None, None),
    }


def failures(name, call, need, good, bad):
    """Every case of one wrapper -> what went wrong (empty: all is as it must be)."""
    d_q, d_off, _ = batch()
    assert d_q.numel() == sum(len(q) for q in QUERIES)            # the sizes above are for the tensors that are passed
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    wrong = []

    def refused(what, q, o, w, out):
        try:
            call(q, o, w, out)
        except RuntimeError as e:
            if "libtvz error" in str(e) and (name, what) not in LEFT_TO_THE_LIBRARY:
                wrong.append(f"{what}: refused by the library, not before it: {e}")
        else:
            wrong.append(f"{what}: accepted")
        torch.cuda.synchronize()
        if any(bool((t != SENTINEL).any()) for t in (out if isinstance(out, tuple) else (out,)) if t is not None):
            wrong.append(f"{what}: an output was written")

    fresh = good if good is not None else (lambda: None)
    refused("float32 queries", d_q.float(), d_off, ws, fresh())
    refused("int32 offsets", d_q, d_off.int(), ws, fresh())
    refused("queries on the CPU", d_q.cpu(), d_off.cpu(), ws, fresh())
    refused("a workspace one byte short", d_q, d_off, ws[:need - 1], fresh())
    if bad is not None:
        refused("a mis-shaped output", d_q, d_off, ws, bad())
    try:
        call(d_q, d_off, ws, fresh())
        torch.cuda.synchronize()
    except RuntimeError as e:
        wrong.append(f"a workspace of exactly {need} bytes: {e}")
    return wrong
