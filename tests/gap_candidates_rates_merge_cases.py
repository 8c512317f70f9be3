"""Hand-made lists for the tvz_align_candidates_rates_merge tests (tests/test_gap_candidates_rates_shards_cpu.py holds the
host merge against the reference on them, tests/test_gap_candidates_rates_merge_gpu.py the kernel).  Plain data, no code
under test.

A case is an int32 array [R, Q, C + 1, 3]: R lists of one call, rows (video_id, best, rate_index) with best in 0..4,095
and rate_index in 0..7, the padding (-1, 0, 0) behind them, then the row (-1, total, 0).  A list names an id at most
once, as the local call writes it; the SAME id may stand in several lists."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
MAX_ID, MAX_BEST, MAX_RATE = (1 << 31) - 1, 4095, 7


def a_list(rows, c, total=None, keep_order=False):
    """(video_id, best, rate_index) triples -> the c + 1 rows of a list: the c best (or, with keep_order, the first c as
    they stand: an unsorted list), padding, the total (default: how many triples there were)"""
    if not keep_order:
        rows = sorted(rows, key=lambda r: (-r[1], r[0]))
    out = list(rows[:c]) + [(-1, 0, 0)] * (c - min(len(rows), c))
    return out + [(-1, len(rows) if total is None else total, 0)]


def block(per_query_lists, c, keep_order=False):
    """per_query_lists[q][r] = (rows, total) -> int32 [R, Q, c + 1, 3]"""
    Q, R = len(per_query_lists), len(per_query_lists[0])
    out = np.zeros((R, Q, c + 1, 3), dtype=np.int32)
    for q, lists in enumerate(per_query_lists):
        assert len(lists) == R
        for r, (rows, total) in enumerate(lists):
            out[r, q] = a_list(rows, c, total, keep_order)
    return out


def random_case(seed, R, Q, c, fill="mixed", id_pool=None, max_best=9, shuffle=False):
    """Bests from a small range and ids from a pool of about 1.5 R c / 2: an id stands in several lists more often than
    not, with equal and with different bests, and ties within and across the lists are plenty.  `fill`: "full" (every list
    c rows), "empty", "short" (fewer than c rows each), "mixed".  `shuffle`: the rows of a list in random order."""
    rng = np.random.default_rng(seed)
    pool = id_pool if id_pool is not None else max(3 * R * c // 4, 2 * c + 4)
    queries = []
    for q in range(Q):
        lists = []
        for r in range(R):
            n = {"full": c, "empty": 0, "short": int(rng.integers(0, c)), "mixed": int(rng.integers(0, c + 1))}[fill]
            ids = rng.choice(pool, size=n, replace=False)                          # distinct within a list
            best = rng.integers(1, max_best + 1, size=n)
            rate = rng.integers(0, MAX_RATE + 1, size=n)
            rows = [(int(v), int(b), int(i)) for v, b, i in zip(ids, best, rate)]
            if shuffle:
                rows = sorted(rows, key=lambda r: (-r[1], r[0]))[:c]
                rows = [rows[i] for i in rng.permutation(len(rows))]
            lists.append((rows, int(n + rng.integers(0, 50))))
        queries.append(lists)
    return block(queries, c, keep_order=shuffle)


def hand_made():
    """-> dict name -> the case"""
    cases = {}
    # every size the issue names: n_lists 1, 2, 3, 8, 16 x C 1, 16, 63, 64 x Q 1, 5
    seed = 300
    for R in (1, 2, 3, 8, 16):
        for c in (1, 16, 63, 64):
            for Q in (1, 5):
                seed += 1
                cases[f"mixed_R{R}_C{c}_Q{Q}"] = random_case(seed, R, Q, c)
    # all 16 lists full of DISTINCT ids: 1,024 rows, none repeats
    distinct = [[([(1000 * r + 7 * j, 1 + (r * 64 + j) % 9, (r + j) % 8) for j in range(64)], None) for r in range(16)]]
    cases["all_full_distinct_1024_rows"] = block(distinct, 64)
    # all 16 lists hold the SAME 64 ids: 64 rows come out, each at its largest best and that best's smallest rate index
    same = [[([(5 * j + 1, 1 + (r * 7 + j * 3) % 11, (r * 3 + j) % 8) for j in range(64)], None) for r in range(16)],
            [([(j, 4, (r + 5) % 8) for j in range(64)], None) for r in range(16)]]      # ... and all of them equal: rate 0
    cases["all_lists_hold_the_same_64_ids"] = block(same, 64)
    cases["all_full_random"] = random_case(7, 16, 3, 64, "full")
    cases["all_full_wide"] = random_case(8, 16, 2, 64, "full", id_pool=1 << 30, max_best=MAX_BEST)
    cases["all_empty"] = random_case(9, 16, 2, 64, "empty")
    cases["all_empty_C1"] = random_case(9, 3, 2, 1, "empty")
    cases["two_lists_C1"] = block([[([(4, 2, 1)], None), ([(4, 2, 0)], None)], [([(4, 2, 1)], None), ([(3, 2, 6)], None)]], 1)
    cases["shorter_than_C"] = random_case(12, 8, 4, 63, "short")
    cases["shorter_than_C_16"] = random_case(13, 16, 4, 16, "short")
    # one id in two lists with equal best and rate indexes 5 and 2: the output says 2 - whichever list comes first
    cases["equal_best_smaller_rate_index"] = block([[([(50, 6, 5), (10, 3, 0)], None), ([(50, 6, 2), (11, 3, 1)], None)],
                                                    [([(50, 6, 2), (10, 3, 0)], None), ([(50, 6, 5), (11, 3, 1)], None)]], 16)
    # one id whose larger best is in the LATER list, at a larger rate index: the best wins, with its own index
    cases["larger_best_in_the_later_list"] = block([[([(50, 3, 0), (10, 5, 1)], None), ([(9, 2, 0)], None),
                                                     ([(50, 8, 6), (11, 3, 1)], None)]], 16)
    # a tie group that straddles rank C: 5 rows of best 9, then 40 ids of best 4 spread over 3 lists - 10 of them in two
    # lists -, C = 16: the lowest 11 ids of the 40 are kept, wherever they stand
    ids = np.random.default_rng(3).permutation(40) + 100
    tie = [[(int(v), 4, int(v) % 8) for v in ids[r::3]] for r in range(3)]
    tie[0] += [(int(v), 4, 7) for v in ids[1::3][:5]] + [(int(v), 3, 0) for v in ids[2::3][:5]]
    tie[1] += [(7, 9, 0), (3, 9, 1)]
    tie[2] += [(5, 9, 2), (900, 9, 3), (1, 9, 4)]
    cases["tie_straddles_C"] = block([[(t, None) for t in tie]], 16)
    # unsorted lists: there is no sortedness precondition
    cases["unsorted_lists"] = random_case(31, 8, 5, 16, "mixed", shuffle=True)
    cases["unsorted_lists_full"] = random_case(32, 16, 2, 64, "full", shuffle=True)
    cases["unsorted_by_hand"] = block([[([(-1, 0, 0), (8, 1, 0), (2, 9, 3), (-1, 0, 0), (8, 1, 0)][:4], 3),
                                        ([(2, 9, 1), (7, 1, 2), (8, 4095, 7)], 3)]], 4, keep_order=True)
    # the word's packing: ids 0 and 2^31 - 1, best 0 and 4,095, rate index 7
    cases["extreme_fields"] = block([[([(0, MAX_BEST, 7), (MAX_ID, MAX_BEST, 7), (1, 0, 7), (MAX_ID - 1, 0, 0)], None),
                                      ([(MAX_ID, MAX_BEST, 0), (0, 0, 0), (MAX_ID - 1, 0, 7), (2, 1, 7)], None)],
                                     [([(MAX_ID, 0, 7)], None), ([(0, 0, 7)], None)]], 8)
    # the totals.  (A negated zero is INT32_MIN, which on the way in is a refusal: a negative total that is no refusal
    # has |t| >= 1, so the merge itself can only write INT32_MIN for a refused query.)
    rows = [(1, 3, 0), (2, 2, 1)]
    cases["totals_plain"] = block([[(rows, 5), (rows, 70000), ([], 0)]], 4)
    cases["totals_one_negative"] = block([[(rows, 5), (rows, -4097), ([], 0)], [(rows, -1), ([], 0), ([], 0)]], 4)
    cases["totals_saturate"] = block([[(rows, INT32_MAX), (rows, INT32_MAX), (rows, 12)],
                                      [(rows, INT32_MAX), ([], 0), ([], 0)],
                                      [(rows, INT32_MAX - 1), ([], 1), ([], 0)],
                                      [(rows, INT32_MAX - 1), ([], 2), ([], 0)]], 4)
    cases["totals_saturate_negative"] = block([[(rows, -INT32_MAX), (rows, INT32_MAX), (rows, 12)],
                                               [(rows, INT32_MAX), (rows, INT32_MAX), (rows, -1)],
                                               [(rows, -INT32_MAX), ([], 0), ([], 0)]], 4)
    cases["totals_16_lists_saturate"] = block([[(rows, INT32_MAX)] * 16, [(rows, 1 << 27)] * 16,
                                               [(rows, (1 << 27) - 1)] * 16], 2)
    cases["refused_in_one_list"] = block([[(rows, 2), ([], INT32_MIN), (rows, 2)], [(rows, 2), (rows, 2), (rows, 2)],
                                          [([], INT32_MIN)] * 3, [(rows, -5), (rows, 2), ([], INT32_MIN)]], 4)
    return cases


def twenty_lists():
    """20 lists, for the merge in groups of 16 + 4: ids repeat across the groups, a negative total in the second group,
    a refused query"""
    b = random_case(21, 20, 4, 16, "mixed")
    b[18, 1, 16, 1] = -int(abs(b[18, 1, 16, 1])) - 1
    b[3, 2, 16, 1] = INT32_MIN
    b[3, 2, :16] = (-1, 0, 0)
    return b
