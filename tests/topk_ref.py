"""The reference of the top-k family (include/tvz.h: tvz_topk, tvz_topk_shard, tvz_topk_merge, the pair merge behind
tvz_match_topk's delta table, and the paragraph at tvz_match_tol_sharded on refused queries), in plain Python on
lists of int tuples - a sorted() and a sum, nothing that could share a bug with the kernels.

An entry is (video_id, count, kth).  Order: ascending (kth, video_id, count).  video_id < 0 is padding."""

KTH_NEVER = 0x7FFFFFFF
INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31
PAD = (-1, 0, KTH_NEVER)


def order_key(e):
    return (e[2], e[0], e[1])


def best(entries, k):
    """The k best of the non-padding entries, padded to k rows."""
    rows = sorted((tuple(e) for e in entries if e[0] >= 0), key=order_key)[:k]
    return rows + [PAD] * (k - len(rows))


def select(entries, n_reported, cap, k, shard_row):
    """tvz_topk (one list; n_reported None = all `cap` entries) / tvz_topk_shard (shard_row): the k rows of the first
    min(max(n_reported, 0), cap) entries; with shard_row a row (-1, t, KTH_NEVER) follows, t = n_reported, negated when
    n_reported > cap (the list was truncated); INT32_MIN (a refused query) passes through unchanged."""
    n = cap if n_reported is None else n_reported
    rows = best(entries[:min(max(n, 0), cap)], k)
    if shard_row:
        rows.append((-1, -n if n > cap else n, KTH_NEVER))
    return rows


def select_lists(lists, lists_n, cap, k):
    """tvz_topk over several lists: the k best of the valid prefixes of all of them."""
    ent = []
    for i, lst in enumerate(lists):
        n = cap if lists_n is None else lists_n[i]
        ent += list(lst[:min(max(n, 0), cap)])
    return best(ent, k)


def merge(blocks, k, pair_cap=None):
    """tvz_topk_merge of R blocks of k + 1 rows (the last one (-1, n, KTH_NEVER)) -> (rows, total).  total = the sum of
    |n| over the ranks, clamped to INT32_MAX, negated if any rank's n was negative; the pair merge behind a delta table
    (pair_cap = the call's hit capacity) also negates it when the sum exceeds pair_cap."""
    ent, total, neg = [], 0, False
    for b in blocks:
        assert len(b) == k + 1
        ent += list(b[:k])
        n = b[k][1]
        total += abs(n)
        neg = neg or n < 0
    if pair_cap is not None and total > pair_cap:
        neg = True
    total = min(total, INT32_MAX)
    return best(ent, k), (-total if neg else total)
