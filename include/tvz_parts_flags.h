/*
 * tvz_parts_flags.h — tvz_align_parts with a flags argument: every aligned part of a named stored video with the votes
 * counted over TWO ADJACENT BINS (libtvz.so, gfx950).
 *
 * New exports beside include/tvz.h and the tvz_gap*.h headers; nothing declared there changes (TVZ_VERSION stays 404).
 *
 * WHY.  tvz_align_parts (include/tvz.h) counts single bins.  A remuxed copy, or one re-timed to another frame grid,
 * sends about half of its votes to bin b and half to b + 1 (TVZ_ALIGN_TWO_BINS, include/tvz.h), so the refinement behind
 * a two-bin search - or behind the candidate ids of tvz_gap.h - scored such a copy at half its votes.  These two calls
 * are tvz_align_parts and tvz_align_parts_shards with `uint32_t flags` inserted behind max_parts.
 *
 *   flags == 0                  : tvz_align_parts's output bit for bit, through the same kernels.
 *   flags == TVZ_ALIGN_TWO_BINS : the semantics below.
 *   any other bit               : TVZ_ERR_INVALID, "alignment parts: unknown flag bits 0x..", as every call with flags
 *                                 words it (bit 4 is no flag of any call; TVZ_ALIGN_CONTAIN and TVZ_ALIGN_LOCAL are
 *                                 score kinds, and this call has no score).
 *   refusals                    : tvz_align_parts's, in its order and words, with the flags checked BEHIND max_parts and
 *                                 IN FRONT OF eps / max_offset / B: the rate list, min_votes, k, max_query_len,
 *                                 max_parts, the flags, the bins; then the handle, the workspace, the pointers.
 *
 * WITH TVZ_ALIGN_TWO_BINS, for a row at one rate and a part i (everything not named here is tvz_align_parts's):
 *   allowed: for part 0 every pair (key c, index t of the sorted query); for i >= 1 the pairs with t outside every
 *            earlier part's [t_first, t_last] and c outside every earlier part's [c_lo, c_hi].
 *   counts : h_i[b], b in [-B, B], is the ALLOWED pairs that vote into bin b by the unchanged expression,
 *            floor((c - s[t] * rho)/eps + 0.5); outside [-B, B] h_i is 0.  J_i[b] = h_i[b] + h_i[b + 1], so J_i[B] =
 *            h_i[B].
 *   best   : the most J, then the most h[b], then the bin order (smaller |b|, then the negative one): the rule of
 *            TVZ_ALIGN_TWO_BINS in include/tvz.h.  A window whose lower bin is empty never wins.
 *   part 0 : exactly tvz_align_span_topk's contract under TVZ_ALIGN_TWO_BINS: per rate the best window, the rate with
 *            the most J kept (the smaller index on a tie).  Later parts stay at that rate.
 *   P_i    : the allowed pairs that vote into b or into b + 1 - the latter only where b + 1 <= B.  t_first, t_last,
 *            c_lo, c_hi, nq_i and nr_i are defined over P_i exactly as tvz_align_parts defines them.
 *   row    : a part's row is (bin, votes, t_first, t_last, nq, nr) with bin = the window's LOWER bin and votes = J raw:
 *            stored = rate x upload + (bin + 0.5) x eps, within one eps.
 *   n_parts: a part is reported iff J >= min_votes; the first part that fails ends the list, and so does max_parts.
 *   unchanged: the row among the rows of one id (most part-0 votes - J here -, then the earlier row of the table); the
 *            refused, absent and no-pair forms; the layout int32[Q][k][1 + max_parts][6]; every workspace byte.
 *
 * WORKSPACE.  tvz_align_parts_workspace_bytes (include/tvz.h) sizes both calls; there is no sizing export here.
 * MERGE.  tvz_align_parts_merge (include/tvz.h) merges the shards' answers as it is: it orders by part-0 votes,
 * whichever way they were counted.  All lists must come from calls with the same flags.
 * NOT HERE: a flags form of tvz_align_parts_sharded (one process per GPU).
 * Cost: two more LDS reads per bin a row walk touches, and the walk of two bins instead of one per part.
 */
#ifndef TVZ_PARTS_FLAGS_H
#define TVZ_PARTS_FLAGS_H

#include "tvz.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tvz_align_parts (include/tvz.h) with `flags` behind max_parts: 0 or TVZ_ALIGN_TWO_BINS.  Only enqueues. */
int tvz_align_parts_flags(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                          int32_t max_query_len, const int32_t *d_video_ids, int64_t id_stride, int64_t query_id_stride,
                          int32_t k, double eps, double max_offset, const double *h_rates, int32_t n_rates,
                          int32_t min_votes, int32_t max_parts, uint32_t flags, int32_t *d_parts, void *d_workspace,
                          size_t workspace_bytes, void *hip_stream);

/* tvz_align_parts_shards (include/tvz.h) with the same insertion: tvz_align_parts_flags on every handle in turn, handle
 * r's answer into d_blocks[r], then tvz_align_parts_merge -> d_parts.  Refuses what tvz_align_parts_flags refuses, in its
 * order and words, then what tvz_align_parts_shards refuses behind that. */
int tvz_align_parts_flags_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                 const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, const int32_t *d_video_ids,
                                 int64_t id_stride, int64_t query_id_stride, int32_t k, double eps, double max_offset,
                                 const double *h_rates, int32_t n_rates, int32_t min_votes, int32_t max_parts,
                                 uint32_t flags, int32_t *d_blocks, int32_t *d_parts, void *d_workspace,
                                 size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TVZ_PARTS_FLAGS_H */
