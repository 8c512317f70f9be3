/*
 * tvz_gap_rates.h — candidate ids from the cut-gap index for copies played at another speed (libtvz.so, gfx950).
 *
 * New exports beside include/tvz_gap.h; nothing declared there or in tvz.h changes (TVZ_VERSION stays 404).
 *
 * A copy played at the rate rho has stored ~= rho x upload + shift, so the stored GAPS are rho x the upload's gaps.
 * The stored codes of tvz_gap.h stay as they are (made at rate 1); the upload is probed once per rate of a list, with
 * its values scaled, and per stored video the best rate is kept.  The block feeds tvz_align_parts with the same list.
 *
 * PROBES AT RATE i.  The query sorted ascending, NaNs skipped, duplicates kept (tvz_gap.h: QUERY SIDE: s, m);
 * x'_j = s_j * rho_i - ONE IEEE multiplication, rounded on its own (no FMA): the alignment calls' expression.  A
 * positive rate keeps the order and equal values equal.  On x' the query side of tvz_gap.h runs word for word:
 * d = x'[j+1] - x'[j], r = d / gap_eps (one true division), a = floor(r), the 8 choices of a or a + 1 for the three
 * gaps of a position, a choice with an invalid bin dropped.  count_i(q, row) = tvz_gap.h's count of those probes.
 *
 * BEST PER STORED VIDEO.  best(q, id) = the largest count_i over the rates i and over EVERY row of that id;
 * rate_index = the smallest i that reaches it (list the rates by preference).  The id is a CANDIDATE iff
 * best >= min_count and id != exclude_id[q].  An id appears at most ONCE in a query's block, however many rows or
 * rates it hit.  Order: best descending, then video_id ascending.
 */
#ifndef TVZ_GAP_RATES_H
#define TVZ_GAP_RATES_H

#include "tvz_gap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace of tvz_align_candidates_rates (total_query_keys = 0: Q * max_query_len); 0 for arguments the
 * call refuses. */
size_t tvz_align_candidates_rates_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                  int32_t n_rates, int32_t cap, int32_t C);

/* Per query the C stored videos that share the most gap codes with it at the best of n_rates rates.
 *   h_rates  HOST array of n_rates doubles, copied into kernel arguments: the call still only enqueues on hip_stream
 *            (no allocation, no host synchronisation).  Equal rates may repeat.
 *   d_out    int32[Q][C + 1][3], 4-byte aligned (refused otherwise): C rows (video_id, best, rate_index), padded with
 *            (-1, 0, 0), then a row (-1, n_pairs, 0).  n_pairs = the (row, rate) pairs with count_i >= min_count (and
 *            another id than the excluded one), summed over the rates in 64 bits and saturated at INT32_MAX.  It is an
 *            UPPER BOUND on the candidate ids, NOT their count: a row that hits at two rates, or two rows of one id,
 *            count twice.  n_pairs is NEGATED when any rate's hit list overflowed `cap` (`cap` holds per query AND
 *            rate; the C best may then be inexact), and INT32_MIN, with every row padding, for a REFUSED query: one
 *            the plain call refuses (longer than max_query_len, or with more than TVZ_GAP_MAX_PROBES probe slots) is
 *            refused at every rate.
 * A block goes to tvz_align_parts as d_video_ids with query_id_stride = (C + 1) * 3, id_stride = 3, k = C, and the
 * same h_rates.
 * With n_rates = 1, h_rates[0] = 1.0 and a table of distinct ids, columns 0 and 1 of every row equal
 * tvz_align_candidates' block bit for bit, the last row included.
 * Refused before the handle is looked at, in this order: tvz_align_candidates' own refusals in its order (C, cap,
 * min_count, max_query_len); the rate list by the rules and with the messages of tvz_align_rates_topk (n_rates outside
 * 1..TVZ_ALIGN_MAX_RATES: TVZ_ERR_UNSUPPORTED; h_rates NULL, or a rate that is NaN, infinite or <= 0:
 * TVZ_ERR_INVALID); Q * n_rates > 65,535 (TVZ_ERR_UNSUPPORTED: the lookup takes that many probe lists); a NULL handle,
 * Q and the query pointers as every batched call checks them; the workspace (TVZ_ERR_WORKSPACE, with the missing
 * bytes); d_out NULL or not 4-byte aligned (TVZ_ERR_INVALID); then a handle without gap codes (TVZ_ERR_UNSUPPORTED).
 * Nothing is written on a refusal.  Upserts that returned before the call are seen. */
int tvz_align_candidates_rates(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                               int32_t max_query_len, const double *h_rates, int32_t n_rates, int32_t min_count,
                               const int32_t *d_exclude_ids, int32_t cap, int32_t C, int32_t *d_out, void *d_workspace,
                               size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TVZ_GAP_RATES_H */
