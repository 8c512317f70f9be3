"""Hand-made lists for the tvz_align_candidates_merge tests (tests/test_gap_candidates_shards_cpu.py holds the host merge
against the reference on them, tests/test_gap_candidates_merge_gpu.py the kernel).  Plain data, no code under test.

A case is an int32 array [R, Q, C + 1, 2]: R lists of one call, each sorted by the contract's order (count descending,
video_id ascending) with the padding (-1, 0) last, then the row (-1, total)."""
import numpy as np

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
MAX_ID = (1 << 31) - 1


def a_list(rows, c, total=None):
    """(video_id, count) pairs in any order -> the c + 1 rows of a list: the c best, padding, the total (default: how
    many pairs there were)"""
    rows = sorted(rows, key=lambda r: (-r[1], r[0]))
    out = rows[:c] + [(-1, 0)] * (c - min(len(rows), c))
    return out + [(-1, len(rows) if total is None else total)]


def block(per_query_lists, c):
    """per_query_lists[q][r] = (rows, total) -> int32 [R, Q, c + 1, 2]"""
    Q, R = len(per_query_lists), len(per_query_lists[0])
    out = np.zeros((R, Q, c + 1, 2), dtype=np.int32)
    for q, lists in enumerate(per_query_lists):
        assert len(lists) == R
        for r, (rows, total) in enumerate(lists):
            out[r, q] = a_list(rows, c, total)
    return out


def random_case(seed, R, Q, c, fill="mixed", id_pool=4000, max_count=9):
    """Counts from a small range and ids from a small pool: ties in plenty within and across the lists, and now and then
    an equal (id, count) in two lists.  `fill`: "full" (every list c rows), "empty", "one" (list R // 2 full, the rest
    empty), "short" (fewer than c rows each), "mixed"."""
    rng = np.random.default_rng(seed)
    queries = []
    for q in range(Q):
        lists = []
        for r in range(R):
            n = {"full": c + int(rng.integers(0, 40)), "empty": 0, "one": c + 7 if r == R // 2 else 0,
                 "short": int(rng.integers(0, c)), "mixed": int(rng.integers(0, 2 * c + 2))}[fill]
            ids = rng.integers(0, id_pool, size=n)
            cnt = rng.integers(1, max_count + 1, size=n)
            lists.append(([(int(v), int(k)) for v, k in zip(ids, cnt)], None))
        queries.append(lists)
    return block(queries, c)


def hand_made():
    """-> dict name -> the case"""
    cases = {}
    # every size the issue names: n_lists 1, 2, 3, 8, 16 x C 1, 16, 63, 64 x Q 1, 5
    seed = 100
    for R in (1, 2, 3, 8, 16):
        for c in (1, 16, 63, 64):
            for Q in (1, 5):
                seed += 1
                cases[f"mixed_R{R}_C{c}_Q{Q}"] = random_case(seed, R, Q, c)
    cases["all_full_1024_rows"] = random_case(7, 16, 3, 64, "full")
    cases["all_full_wide_counts"] = random_case(8, 16, 2, 64, "full", id_pool=1 << 30, max_count=1 << 20)
    cases["all_empty"] = random_case(9, 16, 2, 64, "empty")
    cases["all_empty_C1"] = random_case(9, 3, 2, 1, "empty")
    cases["one_full_rest_empty"] = random_case(10, 16, 2, 64, "one")
    cases["one_full_rest_empty_R3"] = random_case(11, 3, 2, 16, "one")
    cases["shorter_than_C"] = random_case(12, 8, 4, 63, "short")
    cases["shorter_than_C_16"] = random_case(13, 16, 4, 16, "short")
    # a tie group that straddles rank C: 5 rows of count 9, then 40 rows of count 4 spread over 3 lists, C = 16 - the
    # lowest 11 ids of the 40 are kept, wherever they stand
    ids = np.random.default_rng(3).permutation(40) + 100
    tie = [[(int(v), 4) for v in ids[r::3]] for r in range(3)]
    tie[1] += [(7, 9), (3, 9)]
    tie[2] += [(5, 9), (900, 9), (1, 9)]
    cases["tie_straddles_C"] = block([[(t, None) for t in tie]], 16)
    # equal (id, count) in two lists: both kept; and the same with the pair on the edge of C
    cases["equal_rows_in_two_lists"] = block([[([(50, 6), (10, 3)], None), ([(50, 6), (11, 3)], None)]], 16)
    cases["equal_rows_on_the_edge"] = block([[([(50, 6), (10, 3)], None), ([(50, 6), (9, 3)], None)],
                                             [([(50, 6)], None), ([(50, 6)], None)]], 2)
    cases["equal_rows_C1"] = block([[([(50, 6)], None), ([(50, 6)], None), ([(50, 6)], None)]], 1)
    # equal counts across lists: ids ascending
    cases["equal_counts_ids_ascending"] = block([[([(30, 5), (10, 5)], None), ([(20, 5), (40, 5)], None),
                                                  ([(25, 5), (5, 5), (35, 4)], None)]], 4)
    # the word's packing: ids 0 and 2^31 - 1, count 2^31 - 1
    cases["extreme_ids_and_counts"] = block([[([(0, INT32_MAX), (MAX_ID, INT32_MAX), (0, 1), (MAX_ID, 1)], None),
                                              ([(MAX_ID, INT32_MAX), (1, INT32_MAX), (MAX_ID - 1, 1), (0, 2)], None)],
                                             [([(MAX_ID, 1)], None), ([(0, 1)], None)]], 8)
    # the totals
    rows = [(1, 3), (2, 2)]
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
    """20 lists, for the merge in groups of 16 + 4: ties across the groups, a negative total in the second group"""
    b = random_case(21, 20, 4, 16, "mixed")
    b[18, 1, 16, 1] = -int(abs(b[18, 1, 16, 1])) - 1
    b[3, 2, 16, 1] = INT32_MIN
    b[3, 2, :16] = (-1, 0)
    return b
