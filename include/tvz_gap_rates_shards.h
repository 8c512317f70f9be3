/*
 * tvz_gap_rates_shards.h — the candidate ids of include/tvz_gap_rates.h over a table that is split into shards
 * (libtvz.so, gfx950).
 *
 * New exports beside include/tvz.h, tvz_gap.h, tvz_gap_shards.h and tvz_gap_rates.h; nothing declared there changes
 * (TVZ_VERSION stays 404).
 *
 * Each shard answers the rates call for the SAME call - the same queries, rate list, min_count, exclusions, cap and C,
 * over codes of the same gap_eps - with a block int32[Q][C + 1][3], and the merge of the blocks is the answer of the
 * whole table.
 *
 * THE MERGE, per query.  Every row of every list with video_id >= 0 takes part.  Per video id, `best` is the largest
 * over all rows of the id in all lists and rate_index the smallest among the rows that reach it: an id appears at most
 * ONCE in the output, as in the local contract (the plain merge of tvz_gap_shards.h keeps equal rows; this one does
 * not).  The C largest by (best descending, video_id ascending) are kept, padded with (-1, 0, 0).  The last row is
 * (-1, total, 0) by the totals rule of the plain merge: let t_l be list l's last row's second column; if any t_l is
 * INT32_MIN the query is REFUSED (every row padding, the total INT32_MIN); otherwise the total is the sum of |t_l|,
 * accumulated in 64 bits, saturated at INT32_MAX, and negated if any t_l < 0 (INT32_MIN for a negated 0).
 * There is NO sortedness precondition: the kernel sorts.  RANGE PRECONDITION: best in 0..4,095 and rate_index in 0..7,
 * as both producers (the rates call and this merge) write them.  Rows outside these ranges give unspecified values in
 * that query's rows, never a store outside d_out.
 *
 * EXACTNESS.  The merged block is tvz_align_candidates_rates over the union of the shards' rows, bit for bit, wherever
 * no shard's hit list overflowed `cap` - EVEN WHERE ROWS OF ONE ID LIE IN SEVERAL SHARDS (a service keeps an id in one
 * shard, but this ABI takes any handles, and a rank keeps what it ingested):
 *   - best(q, id) over the table is the maximum of the shards' best(q, id), and the smallest rate index that reaches
 *     the maximum over the table is the smallest among the shards that reach it: the per-id rule above.
 *   - An id that a shard dropped from its C best stood behind C ids of that shard.  Those ids' table-wide maxima are
 *     no smaller than their values in that shard, so at least C ids stand in front of the dropped id's value there.
 *     If that value was the id's table-wide maximum, the id is not among the table's C best, and it is rightly gone:
 *     those C ids are all in that shard's block, and the merge ranks them in front.
 *   - An understated copy of such an id - a smaller value of it that another shard kept - ranks lower still, behind
 *     the same C ids: it cannot enter the merged C best either.  Where the shard that holds the id's maximum kept it,
 *     the per-id rule folds every copy into the one row with the maximum.
 *   - n_pairs counts (row, rate) pairs; every row lives in one shard, so the shards' sum is the table's.
 *   - The rule is associative under regrouping (maximum of maxima, smallest index on a tie, C best of C bests, sums of
 *     sums, "any negative", "any refused"): more than 16 lists are merged in groups of up to 16, and the groups'
 *     answers merged again.
 * Where a shard's list overflowed `cap` the merged total is negative, as the local call's is.
 */
#ifndef TVZ_GAP_RATES_SHARDS_H
#define TVZ_GAP_RATES_SHARDS_H

#include "tvz_gap_rates.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TVZ_GAP_RATES_MERGE_MAX_LISTS 16

/* d_gathered int32[n_lists][Q][C + 1][3] -> d_out int32[Q][C + 1][3], a block like a shard's own: it goes to
 * tvz_align_parts by the strides of tvz_gap_rates.h.  One launch on hip_stream (a block per query); no allocation, no
 * host synchronisation.
 * Nothing is written on a refusal: n_lists outside 1..TVZ_GAP_RATES_MERGE_MAX_LISTS or C outside 1..TVZ_GAP_MAX_C
 * (TVZ_ERR_UNSUPPORTED); Q < 0, a NULL pointer, a pointer that is not 4-byte aligned - all a 12-byte row has -, or
 * d_out overlapping d_gathered (TVZ_ERR_INVALID).  Q = 0: TVZ_OK, no pointer is looked at. */
int tvz_align_candidates_rates_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                                     void *hip_stream);

/* The shards of one process: tvz_align_candidates_rates on every handle in turn on hip_stream, handle r's block into
 * d_blocks[r] (int32[n_shards][Q][C + 1][3]), then the merge into d_out.  ONE workspace sized for one handle
 * (tvz_align_candidates_rates_workspace_bytes) serves all of them.
 * Refused before anything is enqueued: what tvz_align_candidates_rates refuses of its arguments, in its order and
 * words (C, cap, min_count, max_query_len, the rate list, Q x n_rates > 65,535); then n_shards outside 1..16
 * (TVZ_ERR_UNSUPPORTED), a NULL handle or handles on different devices, Q < 0, NULL or misaligned d_blocks / d_out
 * (TVZ_ERR_INVALID), the workspace (TVZ_ERR_WORKSPACE), a handle without gap codes and handles whose gap_eps differ
 * (TVZ_ERR_UNSUPPORTED, naming the two widths). */
int tvz_align_candidates_rates_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                      const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, const double *h_rates,
                                      int32_t n_rates, int32_t min_count, const int32_t *d_exclude_ids, int32_t cap, int32_t C,
                                      int32_t *d_blocks, int32_t *d_out, void *d_workspace, size_t workspace_bytes,
                                      void *hip_stream);

/* Bytes of workspace of tvz_align_candidates_rates_sharded: tvz_align_candidates_rates_workspace_bytes + the rank's own
 * block and max(n_ranks, 1) gathered ones (Q x (C + 1) x 12 bytes each, each region rounded up to 256) + 255 for the
 * base's alignment.  0 where the rates sizing function answers 0, and for n_ranks < 0. */
size_t tvz_align_candidates_rates_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                                          int32_t n_rates, int32_t cap, int32_t C, int32_t n_ranks);

/* One process per GPU: the local tvz_align_candidates_rates into the workspace's own block, ONE ncclAllGather of
 * Q x (C + 1) x 3 int32 per rank - ordered on the communicator with the other sharded calls' collectives -, the merge;
 * every rank gets the same d_out.  The rates call's refusals come first, in its order and words; behind them, still
 * before anything is enqueued: a NULL communicator or d_out (TVZ_ERR_INVALID) and more than 16 ranks
 * (TVZ_ERR_UNSUPPORTED).
 * PRECONDITION: every rank's handle keeps gap codes of the same gap_eps and every rank passes the same rate list; a
 * rank cannot check the others'.
 * This call has run on hardware at ONE rank only: never run on more than one GPU. */
int tvz_align_candidates_rates_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                       int32_t Q, int32_t max_query_len, const double *h_rates, int32_t n_rates,
                                       int32_t min_count, const int32_t *d_exclude_ids, int32_t cap, int32_t C, int32_t *d_out,
                                       void *d_workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TVZ_GAP_RATES_SHARDS_H */
