/*
 * tvz_gap.h — candidate ids for the near-duplicate search from a cut-gap index (libtvz.so, gfx950).
 *
 * New exports beside include/tvz.h; nothing declared there changes (TVZ_VERSION stays 404).
 *
 * A shift moves every cut of a video by the same amount, so the GAPS between consecutive cuts do not move.  Three
 * consecutive gaps, quantised, form a key that is invariant under any shift, local (an excerpt, an insertion or a
 * removal keeps every key away from the edit) and exact-matchable: the handle keeps the keys of its rows in a second
 * table of its own and answers "which stored videos share the most keys with this upload" through the inverted index
 * of tvz_match.  The ids feed tvz_align_parts, which aligns the named pairs instead of sweeping the table.
 *
 * GAP BINS.  Ascending values s[0..m) and gap_eps > 0:  d_i = s[i+1] - s[i] (one IEEE subtraction),
 * r_i = d_i / gap_eps (one true division: no reciprocal, no FMA).  A bin is VALID iff it lies in
 * [0, TVZ_GAP_MAX_BIN], compared on the double (NaN fails).  A CODE is g0 + g1 * 2^17 + g2 * 2^34 of three valid
 * bins: below 2^51, exact as a float64.
 *
 * STORED SIDE.  A row as the handle keeps it (sorted ascending, distinct, NaN dropped, -0.0 folded):
 * b_i = floor(r_i + 0.5).  Position i (i + 3 < len) contributes the code of (b_i, b_i+1, b_i+2) if all three are
 * valid; the row's codes are the SET of these.  Rows of fewer than 4 keys have none.
 *
 * QUERY SIDE.  The query sorted ascending, NaNs skipped, duplicates kept (the alignment calls' s, m):
 * a_i = floor(r_i).  Position i contributes up to 8 PROBES: every choice of a_j or a_j + 1 for each of its three
 * gaps; a choice that contains an invalid bin is dropped.  Hence: a stored position is probed whenever each of its
 * three gaps moved by less than gap_eps / 2.
 *
 * count(q, r) = the probes of q, with multiplicity, that are in row r's code set.  Row r is a CANDIDATE iff
 * count >= min_count and video_id != exclude_id[q].  Order: count descending, then video_id ascending; two rows of one
 * id that are equal in both are identical output rows and both kept.
 */
#ifndef TVZ_GAP_H
#define TVZ_GAP_H

#include "tvz.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TVZ_GAP_BIN_BITS 17
#define TVZ_GAP_MAX_BIN 131071     /* 2^17 - 1 */
#define TVZ_GAP_MAX_PROBES 4095    /* probe slots of a query, 8 (m - 3): queries of up to 514 values pass */
#define TVZ_GAP_MAX_C 64

/* gap_eps > 0 and finite: builds the codes of every current row and keeps them current from then on (upload,
 * upsert, clear, reserve and destroy forward to the code table before they return).  gap_eps = 0 drops them.
 * Negative or NaN: TVZ_ERR_INVALID.  Another gap_eps than the current one rebuilds.  Waits for the matches in
 * flight, as tvz_corpus_build_index does. */
int tvz_corpus_gap_index(tvz_corpus *c, double gap_eps);

/* *gap_eps = the width in force (0: off); out = {rows, codes, indexed rows, delta rows, builds} of the code table,
 * all 0 while off.  Either pointer may be NULL. */
int tvz_corpus_gap_index_stats(tvz_corpus *c, double *gap_eps, int64_t out[5]);

/* Bytes of workspace of tvz_align_candidates (total_query_keys = 0: Q * max_query_len); 0 for arguments the call
 * refuses. */
size_t tvz_align_candidates_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t cap,
                                            int32_t C);

/* Per query the C stored videos that share the most gap codes with it.
 *   d_out  int32[Q][C + 1][2]: C rows (video_id, count), padded with (-1, 0), then a row (-1, n_candidates).
 *          n_candidates is NEGATED when the candidates exceeded `cap` (the C best may then be inexact: the rule of
 *          tvz_match_topk), and INT32_MIN, with every row padding, for a REFUSED query: one longer than
 *          max_query_len, or with more than TVZ_GAP_MAX_PROBES probe slots.
 * A block goes to tvz_align_parts as d_video_ids with query_id_stride = (C + 1) * 2, id_stride = 2, k = C.
 * Refused before the handle is looked at, in this order: C outside 1..TVZ_GAP_MAX_C and cap < C
 * (TVZ_ERR_UNSUPPORTED), min_count < 1 (TVZ_ERR_INVALID), max_query_len > 4,095 (TVZ_ERR_UNSUPPORTED), the
 * workspace (TVZ_ERR_WORKSPACE, with the missing bytes); then a handle without gap codes (TVZ_ERR_UNSUPPORTED).
 * The call only enqueues on hip_stream: no allocation, no host synchronisation.  Upserts that returned before the
 * call are seen. */
int tvz_align_candidates(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                         int32_t max_query_len, int32_t min_count, const int32_t *d_exclude_ids, int32_t cap, int32_t C,
                         int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TVZ_GAP_H */
