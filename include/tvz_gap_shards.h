/*
 * tvz_gap_shards.h — the candidate ids of include/tvz_gap.h over a table that is split into shards (libtvz.so, gfx950).
 *
 * New exports beside include/tvz.h and include/tvz_gap.h; nothing declared there changes (TVZ_VERSION stays 404).
 *
 * Every row of the table lives in exactly one shard.  Each shard answers tvz_align_candidates for the SAME call - the
 * same queries, min_count, exclusions, cap, C and gap_eps - with a block int32[Q][C + 1][2], and the merge of the
 * blocks is the answer of the whole table: its C best are among the union of the shards' C best, and its candidate
 * count is the sum of theirs.  This is exact wherever no shard's candidates exceeded `cap`; where one did, the merged
 * total is negative, as the plain call's is.
 *
 * THE MERGE, per query.  Every row of every list with video_id >= 0 takes part; the output keeps the C largest by
 * (count descending, video_id ascending) - rows equal in both are identical output rows, and all of them are kept -
 * and is padded with (-1, 0).  Let t_l be list l's last row.  If any t_l is INT32_MIN the query is REFUSED: every row
 * padding, the total INT32_MIN.  Otherwise the total is the sum of |t_l|, accumulated in 64 bits, saturated at
 * INT32_MAX, and negated if any t_l < 0 (the totals rule of tvz_topk_merge).  The rule is associative under
 * regrouping: more than 16 lists are merged in groups of up to 16, and the groups' answers merged again.
 * PRECONDITION: each list is sorted by that order, padding last, with counts >= 0 - as tvz_align_candidates and this
 * merge itself write them.  Lists that are not give an unspecified selection of their rows, never a store outside
 * d_out.
 */
#ifndef TVZ_GAP_SHARDS_H
#define TVZ_GAP_SHARDS_H

#include "tvz_gap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TVZ_GAP_MERGE_MAX_LISTS 16

/* d_gathered int32[n_lists][Q][C + 1][2] -> d_out int32[Q][C + 1][2], a block like a shard's own: it goes to
 * tvz_align_parts by the same strides.  One launch on hip_stream; no allocation, no host synchronisation.
 * Nothing is written on a refusal: n_lists outside 1..TVZ_GAP_MERGE_MAX_LISTS or C outside 1..TVZ_GAP_MAX_C
 * (TVZ_ERR_UNSUPPORTED); Q < 0, a NULL pointer, a pointer that is not 8-byte aligned, or d_out overlapping d_gathered
 * (TVZ_ERR_INVALID).  Q = 0: TVZ_OK, no pointer is looked at. */
int tvz_align_candidates_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t C, int32_t *d_out,
                               void *hip_stream);

/* The shards of one process: tvz_align_candidates on every handle in turn on hip_stream, handle r's block into
 * d_blocks[r] (int32[n_shards][Q][C + 1][2]), then the merge into d_out.  ONE workspace sized for one handle
 * (tvz_align_candidates_workspace_bytes) serves all of them.
 * Refused before anything is enqueued: what tvz_align_candidates refuses of its arguments, in its order and words;
 * then n_shards outside 1..16 (TVZ_ERR_UNSUPPORTED), a NULL handle or handles on different devices, Q < 0, NULL or
 * misaligned d_blocks / d_out (TVZ_ERR_INVALID), the workspace (TVZ_ERR_WORKSPACE), a handle without gap codes and
 * handles whose gap_eps differ (TVZ_ERR_UNSUPPORTED, naming the two widths). */
int tvz_align_candidates_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, int32_t min_count,
                                const int32_t *d_exclude_ids, int32_t cap, int32_t C, int32_t *d_blocks, int32_t *d_out,
                                void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* Bytes of workspace of tvz_align_candidates_sharded: tvz_align_candidates_workspace_bytes + the rank's own block and
 * max(n_ranks, 1) gathered ones (Q x (C + 1) x 8 bytes each) + alignment.  0 where the plain sizing function answers
 * 0, and for n_ranks < 0. */
size_t tvz_align_candidates_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t cap,
                                                    int32_t C, int32_t n_ranks);

/* One process per GPU: the local tvz_align_candidates into the workspace's own block, ONE ncclAllGather of
 * Q x (C + 1) x 2 int32 per rank - ordered on the communicator with the other sharded calls' collectives -, the merge;
 * every rank gets the same d_out.  The plain call's refusals come first, in its order and words; behind them, still
 * before anything is enqueued: a NULL communicator or d_out (TVZ_ERR_INVALID) and more than 16 ranks
 * (TVZ_ERR_UNSUPPORTED).
 * PRECONDITION: every rank's handle keeps gap codes of the same gap_eps; a rank cannot check the others'.
 * This call has run on hardware at ONE rank only: never run on more than one GPU. */
int tvz_align_candidates_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                 int32_t Q, int32_t max_query_len, int32_t min_count, const int32_t *d_exclude_ids,
                                 int32_t cap, int32_t C, int32_t *d_out, void *d_workspace, size_t workspace_bytes,
                                 void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TVZ_GAP_SHARDS_H */
