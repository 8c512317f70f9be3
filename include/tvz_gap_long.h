/*
 * tvz_gap_long.h — candidate ids from the cut-gap index for LONG uploads (libtvz.so, gfx950).
 *
 * New exports beside include/tvz_gap.h; nothing declared there or in include/tvz.h changes (TVZ_VERSION stays 404, and
 * tvz_align_candidates keeps refusing a query of more than 514 values).
 *
 * tvz_align_candidates hands a query's probes to the lookup as ONE list, and the lookup takes lists of at most
 * TVZ_GAP_MAX_PROBES = 4,095 slots: 8 slots per position, 511 positions, 514 values.  A film of 90 minutes has 900 to
 * 1,400 cuts.  This call cuts a query of up to TVZ_GAP_LONG_MAX_LEN = 4,095 values into SEGMENTS, looks every segment
 * up as a list of its own, and sums what the segments found per stored video.
 *
 * The gap bins, the stored side and the query side (s, m, 8 probes per position) are tvz_gap.h's, word for word.
 *
 * SEGMENTS.  The positions 0 .. m - 4 of a query are cut into segments of TVZ_GAP_LONG_SEG_POSITIONS = 511
 * consecutive positions (4,088 slots: the most whole positions that fit in 4,095).  Segment s holds the positions
 * [511 s, min(511 (s + 1), m - 3)).  S(m) = ceil((m - 3) / 511): 1 up to m = 514, 2 from 515, 3 from 1,026, 9 at
 * 4,095.  A call has S_max = S(min(max_query_len, 4095)) probe lists per query (at least 1); the lists of a query
 * beyond its own S(m) are empty.
 *
 * COUNTS.  c_s(q, row) = tvz_gap.h's count restricted to the probes of segment s.
 * count(q, id) = the sum over the segments s and over EVERY row of that id of c_s(q, row), taking only the terms with
 * c_s >= min_count: min_count holds per segment and per row, as it does in the lookup.  The id is a CANDIDATE iff that
 * sum is positive (hence at least min_count) and id != exclude_id[q].  An id appears at most once in a query's block.
 * Order: count descending, then video_id ascending.
 * Two consequences:
 *   - for m <= 514 (one segment) over a table of distinct ids, the block equals tvz_align_candidates' block bit for
 *     bit, the last row included;
 *   - against the whole-query count of tvz_gap.h a row loses at most min_count - 1 per segment: with S = S(m),
 *     count_whole - S (min_count - 1) <= count_long <= count_whole for a table of distinct ids.
 */
#ifndef TVZ_GAP_LONG_H
#define TVZ_GAP_LONG_H

#include "tvz_gap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TVZ_GAP_LONG_SEG_POSITIONS 511  /* positions of a segment: 8 x 511 = 4,088 probe slots */
#define TVZ_GAP_LONG_MAX_LEN 4095       /* the longest query: 9 segments */
#define TVZ_GAP_LONG_LDS_ENTRIES 2048   /* a query whose hit lists hold at most this many entries is folded in LDS (a
                                           table of twice as many slots), a longer one in the caller's workspace */

/* Bytes of workspace of tvz_align_candidates_long (total_query_keys = 0: Q * max_query_len); 0 for arguments the call
 * refuses.  Per probe list (Q * S_max of them) a hit list of cap x 12 bytes; per query value the sorted copy and eight
 * probe slots (76 bytes: the segments partition the positions, they do not multiply them); where S_max * cap is above
 * TVZ_GAP_LONG_LDS_ENTRIES, per query a table of 8-byte slots, the next power of two at or above 2 * S_max * cap. */
size_t tvz_align_candidates_long_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t cap,
                                                 int32_t C);

/* Per query the C stored videos with the largest count(q, id) above.  The arguments are tvz_align_candidates'.
 *   d_out  int32[Q][C + 1][2] in that call's layout: C rows (video_id, count), padded with (-1, 0), then a row
 *          (-1, n).  n = the number of distinct candidate ids when no segment's hit list overflowed `cap` - cap holds
 *          per query and per segment.  If any list overflowed, n = -(the sum over the segments of their true hit
 *          counts), summed in 64 bits and saturated (tvz_match_topk's rule); the C best may then be inexact, but every
 *          reported id is a candidate and no reported count is above its true count.  INT32_MIN, with every row
 *          padding, for a REFUSED query: one longer than max_query_len.
 * The block goes to tvz_align_parts (query_id_stride = (C + 1) * 2, id_stride = 2, k = C) and to
 * tvz_align_candidates_merge as it is.
 * Refused, in this order: what tvz_align_candidates refuses of C, cap, min_count and max_query_len (> 4,095), in its
 * order and with its messages; Q * S_max > 65,535 (TVZ_ERR_UNSUPPORTED); S_max * cap * 4,088 > INT32_MAX
 * (TVZ_ERR_UNSUPPORTED: every 32-bit sum is exact by construction); the workspace (TVZ_ERR_WORKSPACE, with the missing
 * bytes); a NULL d_out; then a handle without gap codes (TVZ_ERR_UNSUPPORTED).  Nothing is written on a refusal.
 * The call only enqueues on hip_stream: no allocation, no host synchronisation. */
int tvz_align_candidates_long(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                              int32_t max_query_len, int32_t min_count, const int32_t *d_exclude_ids, int32_t cap, int32_t C,
                              int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TVZ_GAP_LONG_H */
