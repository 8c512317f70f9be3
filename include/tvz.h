/*
 * tvz.h — C ABI of libtvz.so, the MI355X (gfx950) duplicate-detection core.
 *
 * The reference (infraheads/tvidz) has NO FFI / plugin boundary on this path.
 * Its two seams are
 *   (1) a child process:  ffmpeg -vf select=gt(scene\,0.3),showinfo   whose
 *       stderr is text-parsed             inspector/app.py:202-232
 *   (2) a Python function: db.find_duplicates(new_timestamps, min_match=5)
 *       -> [(video_id, match_count)]       inspector/db.py:76-94,
 *       driven per new cut by               inspector/app.py:234-255
 * Each entry point below cites the seam it replaces.  Everything is plain C:
 * pointers + sizes, no torch / C++ types.  `d_` = device (HBM) pointer,
 * `h_` = host pointer.  `hip_stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  All functions are re-entrant and the library
 * keeps NO process-global mutable state: kernel-shape / algorithm choices are
 * per-call arguments, carried stream state lives in caller-owned device
 * memory, and the only shared mutable objects are the tvz_corpus / tvz_comm
 * handles (internally locked).  Hot calls allocate nothing: scratch is a
 * caller-provided workspace sized by the *_workspace_bytes functions.
 *
 * Error convention: 0 on success, negative tvz_status otherwise; the message
 * is in tvz_last_error() (thread-local).  The Python shim raises
 * RuntimeError(msg) so failures land in the same `except Exception` as the
 * reference's (inspector/app.py:303).
 */
#ifndef TVZ_H
#define TVZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVZ_VERSION 404 /* 0.4.4: tvz_corpus_index_layout, a read-only query of what the index build made (0.4.3 (unchanged by tvz_corpus_tol_index / tvz_corpus_tol_index_stats: new exports only, nothing existing changes): tvz_match_tol_topk / tvz_match_tol_sharded, the tolerant sweep keeps the per-shard top-k itself (0.4.2: tvz_find_duplicates_tol / tvz_match_tol, the opt-in tolerant match (0.4.1: tvz_align takes its output capacity and reports the row count (0.4.0: the index answers every min_match >= 1; tvz_match_topk keeps the top-k inside the lookup; tvz_match_topk_shards)))) */

typedef enum tvz_status {
    TVZ_OK = 0,
    TVZ_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, ...) */
    TVZ_ERR_HIP = -2,         /* a HIP runtime call failed */
    TVZ_ERR_NOMEM = -3,       /* device or host allocation failed */
    TVZ_ERR_UNSUPPORTED = -4, /* shape outside what the kernels handle */
    TVZ_ERR_WORKSPACE = -5,   /* caller-provided workspace too small */
    TVZ_ERR_COMM = -6         /* RCCL missing or a collective failed */
} tvz_status;

#define TVZ_KTH_NEVER 0x7fffffff /* kth_hit_idx of a candidate that never reaches min_match */

int tvz_version(void);
const char *tvz_last_error(void);

/* ------------------------------------------------------------------------
 * Scene-cut scoring   — replaces the arithmetic reached through
 * inspector/app.py:202-209 (ffmpeg `select=gt(scene,0.3)`; upstream
 * libavfilter/f_select.c get_scene_score + scene_sad.c).
 * ------------------------------------------------------------------------ */

/* Bytes of scratch the scene entry points need for a batch of up to T frames. */
size_t tvz_scene_workspace_bytes(int64_t T, int32_t H, int32_t W);

/* Stream state: what get_scene_score carries from one frame to the next (the
 * previous frame and prev_mafd), kept in DEVICE memory so that a stream scored
 * in micro-batches needs no host round trip between batches and a chain of
 * batches can be captured in one HIP graph.  The caller owns a buffer of
 * tvz_scene_state_bytes() bytes (256-byte aligned), resets it once per video
 * and passes it to every tvz_scene_scores_* call of that video; each call READS
 * the predecessor (frame + mafd) from it and WRITES its own last frame + mafd
 * back.  bytes_per_sample: 1 (8-bit) or 2 (9..16-bit luma in uint16). */
size_t tvz_scene_state_bytes(int32_t H, int32_t W, int32_t bytes_per_sample);
int tvz_scene_state_reset(void *d_state, void *hip_stream);

/* Kernel-shape override for A/B runs, PER CALL (there is no global knob):
 * 0 = automatic; otherwise U | (tc << 8) | TVZ_SHAPE_NO_NT where U in {1,2,4,8} is the strip
 * width (16-byte loads per lane and frame) and tc the frames per time chunk (8,16,32 or a
 * multiple of 64).  Results never depend on it. */
#define TVZ_SHAPE_AUTO 0u
#define TVZ_SHAPE_NO_NT (1u << 30)
#define TVZ_SHAPE(U, tc) ((uint32_t)(U) | ((uint32_t)(tc) << 8))

/* Luma sum of absolute differences between consecutive frames of a batch.
 *   d_luma : uint8 luma planes, frame t at d_luma + t*frame_stride_bytes,
 *            row y at + y*row_stride_bytes, W bytes per row.
 *   d_sad_out[T] : sad[0] = 0, sad[t] = sum |luma[t] - luma[t-1]|  (exact).
 * Every luma byte is read from HBM once (+1 halo frame per time chunk).
 * Fast path: row_stride == W, base and frame stride 16-byte aligned; anything
 * else takes a slower generic kernel with identical results. */
int tvz_luma_sad_u8(const uint8_t *d_luma, int64_t T, int32_t H, int32_t W,
                    int64_t frame_stride_bytes, int64_t row_stride_bytes,
                    uint64_t *d_sad_out, void *d_workspace, size_t workspace_bytes,
                    void *hip_stream);

/* get_scene_score epilogue over a SAD vector:
 *   mafd  = sad / (W*H) / 2^(bitdepth-8);  diff = |mafd - prev_mafd|
 *   score = clipf((float)(min(mafd, diff) / 100), 0, 1);  selected = score > threshold
 * d_prev_mafd = NULL: element 0 is the first frame of the stream (score 0, and
 * element 1 sees ffmpeg's zero-initialised prev_mafd).
 * d_prev_mafd != NULL (device pointer to one double): the batch continues a
 * stream; sad[0] is a real SAD against the previous batch's last frame and
 * *d_prev_mafd is that batch's last mafd.  d_score / d_mafd may be NULL. */
int tvz_scene_select(const uint64_t *d_sad, int64_t T, int32_t H, int32_t W,
                     int32_t bitdepth, double threshold, const double *d_prev_mafd,
                     uint8_t *d_selected, double *d_score, double *d_mafd, void *hip_stream);

/* Fused batch call: luma -> sad, mafd, score, selected (+ the compacted cut list).
 *   d_state (nullable): stream state (above).  NULL = a self-contained batch whose frame 0 is
 *       the first frame of a stream (score 0).  Non-NULL: frame 0 is scored against the state's
 *       frame unless the state was just reset, and the state is advanced to this batch's end.
 *   d_cuts (nullable): int32[1 + cuts_cap]; [0] = number of selected frames of the batch, then
 *       their indices in ascending order (the first cuts_cap of them) - ONE small device-to-host
 *       copy per micro-batch gives the host everything showinfo would have printed.
 *   Any of d_sad_out / d_score / d_mafd may be NULL; d_selected is required with d_cuts.
 * Enqueues kernels only (no allocation, no synchronisation): graph-capturable. */
int tvz_scene_scores_u8(const uint8_t *d_luma, int64_t T, int32_t H, int32_t W,
                        int64_t frame_stride_bytes, int64_t row_stride_bytes, void *d_state,
                        int32_t bitdepth, double threshold, uint64_t *d_sad_out, double *d_mafd,
                        double *d_score, uint8_t *d_selected, int32_t *d_cuts, int32_t cuts_cap,
                        void *d_workspace, size_t workspace_bytes, uint32_t shape,
                        void *hip_stream);

/* The same for 9..16-bit luma stored as uint16 (yuv420p10 etc.): ffmpeg's ff_scene_sad16_c sums
 * |a-b| over uint16 samples and get_scene_score divides mafd by 2^(bitdepth-8).  Strides are in
 * BYTES. */
int tvz_scene_scores_u16(const uint16_t *d_luma, int64_t T, int32_t H, int32_t W,
                         int64_t frame_stride_bytes, int64_t row_stride_bytes, void *d_state,
                         int32_t bitdepth, double threshold, uint64_t *d_sad_out, double *d_mafd,
                         double *d_score, uint8_t *d_selected, int32_t *d_cuts, int32_t cuts_cap,
                         void *d_workspace, size_t workspace_bytes, uint32_t shape,
                         void *hip_stream);

/* ------------------------------------------------------------------------
 * Timestamp corpus   — device image of the `video_timestamps` table
 * (inspector/db.py:21-27): one row = (video_id, float8[] timestamps).
 * ------------------------------------------------------------------------ */
typedef struct tvz_corpus tvz_corpus;

int tvz_corpus_create(tvz_corpus **out, int device);
/* Must not run concurrently with any other call on the same handle. */
int tvz_corpus_destroy(tvz_corpus *c);

/* Pre-size the device arena / row table / single-query staging for at least this many rows and
 * keys, so later upserts and queries allocate nothing (upload reserves 2x its input itself). */
int tvz_corpus_reserve(tvz_corpus *c, int64_t n_rows, int64_t n_keys);

/* Replace the whole corpus (the `session.query(VideoTimestamps).all()` of
 * db.py:83 done once instead of per call).  Row r owns
 * h_keys[h_offsets[r] .. h_offsets[r+1]).  Rows need not be sorted or unique;
 * NaN keys are dropped (NaN == x is false), -0.0 is folded into +0.0. */
int tvz_corpus_upload(tvz_corpus *c, const int32_t *h_video_ids, const int64_t *h_offsets,
                      const double *h_keys, int64_t n_rows, int64_t n_keys);

/* add_timestamps (db.py:43-64): replace the first row of `video_id` with the
 * new list, or append a row if the video has none.  Does NOT wait for matches
 * in flight: the new keys go to fresh arena space and the 16-byte row entry is
 * swapped by a stream-ordered device write, so a concurrent match sees the old
 * or the new row, never a mix; every match ENQUEUED after this call returns
 * sees the new row (read-your-writes, as a committed db.py:58-62 would give). */
int tvz_corpus_upsert(tvz_corpus *c, int32_t video_id, const double *h_keys, int64_t n);

/* `/admin/clear-db` (app.py:325-333).  Matches already enqueued keep sweeping the rows they were
 * launched with, unchanged: the arena is reused by later upserts only after those matches (the
 * mutation stream waits for them on the device; the host does not). */
int tvz_corpus_clear(tvz_corpus *c);

int tvz_corpus_stats(tvz_corpus *c, int64_t *n_rows, int64_t *n_keys, int64_t *arena_keys);

/* Inverted index (no reference counterpart: db.py:83 has no index and reads the whole table per
 * call).  The handle keeps, next to the row table, key -> rows posting lists over the rows as
 * they were at the last build - ONE directory over the distinct keys of all rows (one probe per
 * query timestamp), the postings of a key contiguous and ordered by sub-index of 16384 rows - and a
 * DELTA table with the current entry of every row added or replaced since.  A match with
 * min_match 1..5 is then a lookup (cost ~ postings of the query's keys, independent of the corpus
 * size) + a sweep of the delta table; results are identical to a full sweep (every row is in
 * exactly one of the two).
 * Built by tvz_corpus_upload and by this call (both wait for matches in flight).  Rebuilt IN THE
 * BACKGROUND - by the upserting thread that crosses the threshold, into a shadow generation that is
 * swapped in under the handle's lock; matches and other upserts go on meanwhile, no reader waits -
 * when a corpus grown by upserts reaches 4096 rows and when the delta table holds
 * max(512, indexed rows / 256) rows.  Both generations are sized with the corpus reservation
 * (tvz_corpus_reserve / upload), so rebuilds allocate only once the corpus has outgrown it.
 * A corpus with >= 2^32 keys (per GPU) gets no index and is swept. */
int tvz_corpus_build_index(tvz_corpus *c);
/* indexed rows / rows in the delta table / postings / distinct keys (directory entries in use) /
 * builds so far (any may be NULL); all 0 while there is no index. */
int tvz_corpus_index_stats(tvz_corpus *c, int64_t *n_indexed_rows, int64_t *n_delta_rows,
                           int64_t *n_postings, int64_t *n_distinct_keys, int64_t *n_builds);
/* The directory of a handle of ONE sub-index (up to 16,384 indexed rows) is a table of 128-byte buckets - a key's
 * entry and its postings in one cache line.  out[0] = buckets (0: the handle has no index, or more than one
 * sub-index: the open-addressing directory), out[1] = keys that do not live in their home bucket, out[2] = how far
 * the farthest of them walked (buckets), out[3] = keys whose posting list lives in the external area,
 * out[4] = external postings (uint16 units, whole lines), out[5] = sub-indexes. */
int tvz_corpus_bucket_stats(tvz_corpus *c, int64_t out[6]);
/* What the last build made of the open-addressing directory of the current generation (read-only; nothing sets it):
 * out[0] = bytes per directory entry (16 + 2 per sub-index, sub-indexes rounded up to 8), out[1] = log2 of the
 * entries, out[2] = log2 of the entries per slice, out[3] = 1 if the directory was built slice by slice (the
 * partitioned build), 0 if by the count and fill over the whole directory; out[4..7] = the same for the cell
 * directory of tvz_corpus_tol_index (0 while the generation carries none).  All 0 while there is no index and for a
 * handle of one sub-index, whose key directory is the bucket table above. */
int tvz_corpus_index_layout(tvz_corpus *c, int64_t out[8]);

/* ------------------------------------------------------------------------
 * Corpus match   — replaces db.find_duplicates (inspector/db.py:76-94) and
 * the per-prefix loop around it (inspector/app.py:231-255).
 *
 * For every (query q, corpus row r):
 *   count = #{ i : query_q[i] in row_r }                (db.py:86-89; query
 *           multiplicity counts, the row is a set, exact float64 ==)
 *   kth   = index i of the min_match-th such hit        (TVZ_KTH_NEVER if
 *           count < min_match, -1 if min_match <= 0)
 * A pair is a HIT iff count >= min_match (db.py:90) and video_id !=
 * exclude_id[q] (app.py:237).  Hits are appended per query as int32 triples
 * (video_id, count, kth), in unspecified order (as db.py:83 has no ORDER BY).
 * `kth` makes the streaming loop a single call: prefix k+1 is the first prefix
 * on which find_duplicates returns row r  <=>  kth == k.
 * ------------------------------------------------------------------------ */

/* How the corpus is matched, PER CALL (there is no global knob); results never depend on it.
 *   AUTO : INDEX when the handle has one and min_match >= 1 (1..5: kth from the smallest positions kept per
 *          candidate; more: count + a kth fix-up walk).  Otherwise (and for the delta
 *          table): one query (or <= 4 against a small corpus) -> Q1; >= 64 queries x >= 2,100 + 340,000 / Q rows
 *          with min_match 1..2 -> JOIN; else TILE
 *   INDEX: posting-list lookup - one block per query walks its sub-indexes (a small batch: one block per
 *          query and sub-index) - + a sweep of the delta table (error if the handle has no index or
 *          min_match < 1)
 *   Q1   : one corpus sweep per query, the query's keys in a small LDS table, per-lane counters
 *   TILE : one LDS hash table per tile of <= 16 queries
 *   JOIN : device-memory hash join per tile of <= 1024 queries (min_match 1..2; other values take TILE) */
#define TVZ_ALGO_AUTO 0
#define TVZ_ALGO_Q1 1
#define TVZ_ALGO_TILE 2
#define TVZ_ALGO_JOIN 3
#define TVZ_ALGO_INDEX 4
/* Shape of the lookup that keeps the top-k (tvz_match_topk, tvz_match_topk_shards, tvz_match_sharded), OR-ed into
 * `algo`.  By default a block takes TWO queries - their directory probes share one probe phase - when the batch
 * still fills the chip with half as many blocks (Q >= 2048) and the LDS of both fits four blocks per CU (queries of
 * up to ~380 timestamps on a handle of one or two sub-indexes, ~150 at seven); _PAIR asks for it at any batch size
 * (where the LDS allows), _NO_PAIR never.  Same results either way. */
#define TVZ_ALGO_PAIR 0x100
#define TVZ_ALGO_NO_PAIR 0x200
/* On a handle of ONE sub-index (up to 16,384 indexed rows: a rank's share of an 8-way sharded 100k-video table) and
 * queries of up to 512 timestamps the lookup that keeps the top-k gives every query to one WAVE instead of a block
 * (ts_match_wq_topk_kernel: no barriers, every probe of the query in flight at once, the postings in registers
 * between the passes).  _NO_WAVE keeps the block kernel, _WAVE asks for the wave kernel (an error where the handle or
 * the batch does not fit it).  Same results either way. */
#define TVZ_ALGO_WAVE 0x400
#define TVZ_ALGO_NO_WAVE 0x800
/* Which of the two is faster depends on what else the GPU is doing: ONE batch alone is answered sooner by the block
 * kernel (59 against 72 us for 4,096 queries on a 12.5k-row shard: all waves of the wave kernel start their probe
 * bursts together), a STREAM of batches - two or three in flight on their own streams, what tvz_match_sharded's
 * callers run - by the wave kernel, which executes a third fewer instructions (40 against 42 us per batch).  The
 * default is the block kernel; _PREFER_WAVE takes the wave kernel wherever it fits and says nothing where it
 * does not (sharded.RcclShardedMatcher sets it). */
#define TVZ_ALGO_PREFER_WAVE 0x1000

/* Scratch for the batched calls below.  k = 0 for tvz_match (tables of the hash join only);
 * k > 0 adds the hit lists + per-shard top-k block of tvz_match_topk / tvz_match_sharded
 * (and n_ranks gathered blocks for the latter; pass n_ranks = 1 otherwise). */
size_t tvz_match_workspace_bytes(int32_t Q, int32_t max_query_len, int32_t cap, int32_t k,
                                 int32_t n_ranks);
/* ... for a batch that holds queries of MORE than 4,095 timestamps (inspector/db.py:87 has no limit).  Such a query
 * is swept on its own: its sorted distinct keys and their multiplicities are made ON THE DEVICE, in a tail of this
 * workspace - the call allocates nothing and synchronises once (the host has to read the query offsets to learn
 * which queries are long).  tvz_match_workspace_bytes has room for ONE query of max_query_len keys;
 * total_query_keys = the key count of the whole batch (the length of d_queries) makes room for any split of it
 * into long queries.  A call whose workspace is too small for its long queries returns TVZ_ERR_WORKSPACE and says
 * how many bytes they need. */
size_t tvz_match_workspace_bytes_long(int32_t Q, int32_t max_query_len, int32_t cap, int32_t k,
                                      int32_t n_ranks, int64_t total_query_keys);

/* Batched, device-resident form.
 *   d_queries   : float64 keys of all queries back to back
 *   d_q_offsets : int64[Q+1]
 *   d_exclude_ids : int32[Q] or NULL
 *   d_hits      : int32[Q][cap][3] out;  d_hits_n : int32[Q] out = number of
 *                 hits found (may exceed cap; only the first cap are stored)
 *   max_query_len : upper bound on any query's length (sizes the query tables).  If it is NOT an
 *                 upper bound the affected queries get d_hits_n = INT32_MIN.
 *                 Any length is accepted (db.py:87 has no limit).  Up to 4095 the call only enqueues
 *                 kernels.  Above, the batch may hold queries of more than 4095 timestamps: the
 *                 library then reads the offsets back, runs the short queries as usual and sweeps
 *                 every long one on its own (sorted-query search + a kth fix-up pass) - the one
 *                 batched path that synchronises the stream and allocates scratch.  Rare by nature
 *                 (a video with thousands of cuts). */
int tvz_match(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets,
              int32_t Q, int32_t max_query_len, int32_t min_match,
              const int32_t *d_exclude_ids, int32_t cap,
              int32_t *d_hits, int32_t *d_hits_n, void *d_workspace, size_t workspace_bytes,
              int32_t algo, void *hip_stream);

/* Match + per-shard top-k behind ONE call (hit lists stay in the workspace):
 *   d_out : int32[Q][k+1][3] = the k best hits by (kth, video_id, count), padded with
 *           (-1, 0, TVZ_KTH_NEVER), + a row (-1, n_hits, TVZ_KTH_NEVER); n_hits is NEGATED when
 *           the hit list overflowed `cap` (the top-k may then be inexact: re-run with more).
 * On an indexed handle (min_match 1..5, k <= 64, a batch large enough that a block owns its query) the
 * lookup kernel keeps the k best ITSELF: no hit list is written, no top-k kernel runs; rows added or
 * replaced since the index was built are swept and merged in.  The contract is unchanged (n_hits is
 * still negated when it exceeds `cap`), the rows are then the exact k best nevertheless. */
int tvz_match_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets,
                   int32_t Q, int32_t max_query_len, int32_t min_match,
                   const int32_t *d_exclude_ids, int32_t cap, int32_t k, int32_t *d_out,
                   void *d_workspace, size_t workspace_bytes, int32_t algo, void *hip_stream);

/* Host-in / host-out single query: the drop-in for db.find_duplicates.
 * Results sorted by (video_id, count).  *n_out = number of hits (if > cap only
 * cap are returned).  h_out_kth may be NULL.  Any query length is accepted.
 * One kernel launch + one stream synchronisation for queries of <= 4095 timestamps - also when the
 * handle has an index AND rows in the delta table (the streaming driver's call: its own row was
 * upserted a moment ago): lookup and delta sweep are one fused launch - the kernel writes its hits
 * straight into pinned host memory owned by the handle. */
int tvz_find_duplicates(tvz_corpus *c, const double *h_query, int64_t n, int32_t min_match,
                        int32_t exclude_id, int64_t cap, int32_t *h_out_ids,
                        int32_t *h_out_counts, int32_t *h_out_kth, int64_t *n_out);

/* Per-query top-k of hit lists ordered by (kth asc, video_id asc, count asc).
 *   d_lists : int32[n_lists][Q][cap][3]  (n_lists = 1 for a local tvz_match
 *             result; = world size for an all-gathered set of per-shard top-k)
 *   d_lists_n : int32[n_lists][Q] valid counts, or NULL = all cap entries
 *             (entries with video_id < 0 are padding and sort last)
 *   d_topk  : int32[Q][k][3] out, padded with (-1, 0, TVZ_KTH_NEVER). */
int tvz_topk(const int32_t *d_lists, const int32_t *d_lists_n, int32_t n_lists, int32_t Q,
             int32_t cap, int32_t k, int32_t *d_topk, void *hip_stream);

/* Sharded form (one process per GPU): each rank reduces its local hit lists to
 *   d_out : int32[Q][k+1][3] = its k best hits + a row (-1, n_local_hits, TVZ_KTH_NEVER),
 * the ranks all-gather those blocks (RCCL), and every rank merges
 *   d_gathered : int32[n_ranks][Q][k+1][3]  ->  d_topk int32[Q][k][3], d_totals int32[Q]
 * (d_totals = hits over all shards; > k means the merged list is truncated to the k best;
 * NEGATIVE means some shard's hit list overflowed `cap`, so its top-k may be inexact: re-run with
 * a larger cap).  The gathered blocks are what tvz_match_topk / tvz_topk_shard wrote: k rows in
 * ascending (kth, video_id, count) order, padding last - up to 16 ranks and k <= 64 are merged as
 * SORTED lists (a k-way merge, not a selection). */
int tvz_topk_shard(const int32_t *d_hits, const int32_t *d_hits_n, int32_t Q, int32_t cap,
                   int32_t k, int32_t *d_out, void *hip_stream);
/* The shards of ONE process (several handles on one device: service.ShardedCorpus, the one-GPU form of
 * configs[4]): tvz_match_topk on every handle in turn, the blocks written where the merge reads them
 *   d_blocks : int32[n_shards][Q][k+1][3]  (as an all-gather would deliver them)
 * and the merge -> d_topk int32[Q][k][3], d_totals int32[Q] - ONE call for the whole tick (a Python
 * host otherwise re-takes its interpreter lock after every launch; with 16 upload threads busy in the
 * ORM that was ~4 ms per tick against ~0.2 ms of GPU work).  One workspace sized for ONE handle
 * (tvz_match_workspace_bytes(Q, max_query_len, cap, k, 1)) serves all of them: same stream, in order. */
int tvz_match_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                          const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, int32_t min_match,
                          const int32_t *d_exclude_ids, int32_t cap, int32_t k, int32_t *d_blocks,
                          int32_t *d_topk, int32_t *d_totals, void *d_workspace, size_t workspace_bytes,
                          int32_t algo, void *hip_stream);
int tvz_topk_merge(const int32_t *d_gathered, int32_t n_ranks, int32_t Q, int32_t k,
                   int32_t *d_topk, int32_t *d_totals, void *hip_stream);

/* ------------------------------------------------------------------------
 * Multi-GPU corpus match: one process per GPU, the corpus rows sharded over
 * the ranks, ONE RCCL all-gather of the per-shard top-k blocks per query batch.  RCCL is bound at
 * run time (dlopen of librccl.so, the copy already mapped by the process if there is one), so
 * libtvz.so loads on hosts without it; tvz_comm_* then return TVZ_ERR_COMM.
 *   rank 0: tvz_comm_unique_id(id)  -> ship the 128 bytes to the other ranks by any means
 *   every rank, BEFORE or after its first GPU call: tvz_comm_init(&comm, id, nranks, rank, dev)
 * ------------------------------------------------------------------------ */
#define TVZ_UNIQUE_ID_BYTES 128
typedef struct tvz_comm tvz_comm;

int tvz_comm_unique_id(void *out_id /* TVZ_UNIQUE_ID_BYTES */);
int tvz_comm_init(tvz_comm **out, const void *unique_id, int32_t n_ranks, int32_t rank,
                  int32_t device);
int tvz_comm_info(tvz_comm *comm, int32_t *n_ranks, int32_t *rank);
int tvz_comm_destroy(tvz_comm *comm);

/* local tvz_match_topk -> ncclAllGather of int32[Q][k+1][3] on `hip_stream` -> tvz_topk_merge.
 * Every rank gets the same d_topk int32[Q][k][3] and d_totals int32[Q] (see tvz_topk_merge).
 * Workspace: tvz_match_workspace_bytes(Q, max_query_len, cap, k, n_ranks).  Two calls on two
 * streams with two workspaces overlap one batch's collective with the next batch's match. */
int tvz_match_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries,
                      const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                      int32_t min_match, const int32_t *d_exclude_ids, int32_t cap, int32_t k,
                      int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                      size_t workspace_bytes, int32_t algo, void *hip_stream);

/* ------------------------------------------------------------------------
 * Opt-in alignment score.  NOT the reference's verdict: db.py:79 matches
 * exactly; README.md:291 ("0.1 s tolerance") and north_star's "alignment/Jaccard" describe a
 * shift/tolerance-aware comparison, which this reports ALONGSIDE the exact one.  For one query
 * against every corpus row, every (query_i, row_j) difference votes into bins of width eps over
 * [-max_offset, +max_offset] (bin = floor(diff/eps + 0.5)):
 *   d_out : int32[out_rows][5] = (video_id, row_len, best_bin, votes_in_best_bin, votes_in_bin_0)
 * Rows are sets (NaN dropped, -0.0 folded to +0.0); query NaNs are skipped and query duplicates
 * each vote.  `votes` counts (query value, row key) PAIRS: with cuts closer than eps it can exceed
 * min(n, row_len).  best_bin ties: smaller |bin| first, then the negative one; no votes at all ->
 * best_bin 0.  A cut-shifted copy shows as votes ~ min(n, row_len) at best_bin = shift/eps;
 * tolerant Jaccard = v / (n + row_len - v) with v = min(votes, n, row_len).
 * *n_rows = the handle's row count, read under its lock; the first min(out_rows, *n_rows) rows are
 * written, nothing beyond them (rows upserted after the caller sized d_out: call again with room).
 * Needs 2*round(max_offset/eps)+1 <= 4096 bins (else TVZ_ERR_UNSUPPORTED); eps > 0, max_offset >= 0. */
int tvz_align(tvz_corpus *c, const double *d_query, int32_t n, double eps, double max_offset,
              int32_t *d_out, int64_t out_rows, int64_t *n_rows, void *hip_stream);

/* The alignment score for a BATCH of queries with the k best-aligned rows kept inside the sweep: no row per corpus
 * row, nothing that grows with rows or hits.  (TVZ_VERSION unchanged: new exports only.)  For query q and row r the
 * votes and bins are tvz_align's, word for word: the row is a set; query NaNs are skipped, query duplicates vote again;
 * B = floor(max_offset/eps + 0.5); the pair (key c, value x) votes into floor((c - x)/eps + 0.5) when that lies in
 * [-B, B] (ONE IEEE subtraction, ONE true division: no reciprocal, no FMA); best bin = most votes, then smaller |bin|,
 * then the negative one.  Then, with nv = the query's non-NaN values and votes = the votes in the best bin:
 *   v     = min(votes, nv, row_len),  u = nv + row_len - v
 *   score = (v << 20) / u   in 64-bit integer division: the tolerant Jaccard above in 20-bit fixed point,
 *           0 <= score <= 2^20 (u >= v); a host restates it exactly
 *   hit  <=> v >= min_votes and score >= min_score and video_id != exclude_id[q]
 *   order : ascending by the 64-bit word (2^20 - score) << 43 | video_id << 12 | (best_bin + 2048)  (21 + 31 + 12
 *           bits): better score first, then smaller video id; hits with equal words (two rows of one video_id) by
 *           (row_len, votes) ascending; rows equal in all of that are identical output rows and are all kept.
 *   d_out : int32[Q][k+1][4] = the k best hits as (video_id, row_len, best_bin, votes) - votes raw, as tvz_align
 *           reports it -, padding rows (-1, 0, 0, 0), and a last row (-1, n_hits, 0, 0) with the TRUE number of
 *           hits, never negated.  n_hits = INT32_MIN (all rows padding) for a query longer than max_query_len or one
 *           whose sorted copy does not fit the workspace; 0 for an empty corpus, an empty or a NaN-only query.
 * The rows seen are the handle's table at the call (upserts made before the call are seen).  Enqueues only: no
 * allocation, no host synchronisation.  Refusals, nothing written: eps / max_offset as tvz_align (TVZ_ERR_INVALID;
 * TVZ_ERR_UNSUPPORTED for more than 4,096 bins); min_votes < 1 or min_score outside 0..2^20: TVZ_ERR_INVALID; k outside
 * 1..64 or max_query_len > 4,095: TVZ_ERR_UNSUPPORTED; a workspace below the fixed parts + one query of max_query_len
 * values (tvz_align_topk_workspace_bytes(Q, max_query_len, max_query_len, k)): TVZ_ERR_WORKSPACE with the bytes missing.
 * Workspace = tvz_match_tol_workspace_bytes(Q, max_query_len, max(total_query_keys, max_query_len))   (the sorted queries;
 *             total_query_keys = the length of d_queries, 0: Q x max_query_len)
 *           + 4 Q                                                                      (hit totals)
 *           + max(6080, 95 Q) x k x 16                                                  (one kept list - k words and k
 *             payloads - per sweep block: min(rows / 4, 6080 / Q clamped to 95..2048) row blocks per query)
 *           + alignment (each part to 256 B).
 * Cost: per row key one binary search of the sorted query (in LDS) + the votes that count - the query values that
 * vote for a key are one contiguous run of the sorted query -, not queries x row keys, and no pass over the bins. */
size_t tvz_align_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k);
int tvz_align_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                   int32_t max_query_len, double eps, double max_offset, int32_t min_votes,
                   int32_t min_score, const int32_t *d_exclude_ids, int32_t k, int32_t *d_out,
                   void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* The alignment top-k AT ANY SHIFT: tvz_align_topk over up to 2^22 offset bins on either side of zero, for the copy
 * whose cut pattern moved by minutes or hours (an intro cut off, an excerpt, a compilation).  (TVZ_VERSION unchanged:
 * new exports only.)  The contract is tvz_align_topk's, word for word, with three changes:
 *   bins  : B = floor(max_offset/eps + 0.5) may be anything in 0..TVZ_ALIGN_WIDE_MAX_B; more, max_offset = +inf or a
 *           NaN quotient: TVZ_ERR_UNSUPPORTED (eps <= 0, max_offset < 0 or a NaN in either: TVZ_ERR_INVALID, as
 *           before).  The vote is the same floor((c - x)/eps + 0.5) in [-B, B] (ONE IEEE subtraction, ONE true
 *           division); the best bin - most votes, then smaller |bin|, then the negative one - is chosen over the
 *           WHOLE range.
 *   score : flags & TVZ_ALIGN_CONTAIN: u = min(nv, row_len), the containment of the shorter side - a 20-cut excerpt
 *           of a 400-cut film whose cuts all align scores 2^20, where the Jaccard u = nv + row_len - v gives 0.05.
 *           score = (v << 20) / u stays in 0..2^20 (v <= u); flags = 0: the Jaccard.  Any other flag bit:
 *           TVZ_ERR_INVALID.
 *   order : ascending by the tuple (2^20 - score, video_id, best_bin as a signed number, row_len, votes); rows equal
 *           in all five are identical rows and are all kept.  For B <= 2047 that is the order of tvz_align_topk's
 *           word, so with flags = 0 the block equals tvz_align_topk's bit for bit.
 * d_out, n_hits, INT32_MIN for a refused query, k in 1..64, max_query_len <= 4,095, min_votes >= 1, min_score in
 * 0..2^20, the refusals (nothing written), enqueue-only, upserts before the call seen: as tvz_align_topk.
 * Workspace = tvz_match_tol_workspace_bytes(Q, max_query_len, max(total_query_keys, max_query_len))   (the sorted queries)
 *           + 4 Q                                                                      (hit totals)
 *           + max(6080, 95 Q) x k x 20                                                  (one kept list per sweep
 *             block; a kept hit is two 64-bit words - score and video id; bin and row_len - and the 32-bit votes)
 *           + alignment (each part to 256 B).
 * Cost: a row's offset range [bin(c_min, x_max), bin(c_max, x_min)], clipped to [-B, B], is walked in windows of 1,024
 * bins (B <= 2047: one window of all bins, the work of tvz_align_topk); per row key one binary search of the sorted
 * query, then one step per window, and over all windows every (key, value) pair inside [-B, B] votes once - far more
 * votes than the bounded search counts.  TVZ_ALIGN_WIDE_MAX_B bounds a row at 8,193 windows.  These blocks have sharded
 * forms of their own (tvz_align_wide_topk_merge, _shards, _sharded, below); the bounded ones (tvz_align_topk_merge,
 * _shards, _sharded) must not be fed them: their merge rebuilds a 12-bit bin word. */
#define TVZ_ALIGN_WIDE_MAX_B (1 << 22)   /* bins on either side of zero */
#define TVZ_ALIGN_CONTAIN 1u             /* flags: score = v / min(nv, row_len) instead of the Jaccard */

/* TVZ_ALIGN_TWO_BINS: the votes of a row counted over a window of TWO ADJACENT BINS that slides by one bin, for the
 * copy whose true shift lies near a bin's edge: the cuts' jitter (a remux, a re-timing to another frame grid) then
 * sends about half the votes to bin b and half to b + 1, and the best single bin holds half of them.  A flag of
 * tvz_align_wide_topk, tvz_align_rates_topk and tvz_align_span_topk, combined freely with TVZ_ALIGN_CONTAIN and, on the
 * span call, with TVZ_ALIGN_LOCAL (TVZ_ALIGN_CONTAIN | TVZ_ALIGN_LOCAL stays refused, with or without it).  Its value
 * is 8: bit 4 is no flag of any call and stays refused everywhere (TVZ_ERR_INVALID), as every other unknown bit.
 * (TVZ_VERSION unchanged; a library built before the flag existed refuses it with TVZ_ERR_INVALID.)  With the flag
 * clear every output of every call is what it was.  With it, for a row at one rate:
 *   counts : h[b], b in [-B, B], is the votes of bin b as above - the same expression, the same single subtraction and
 *            single division, the same multiplication by the rate with no FMA -; outside [-B, B] h is 0.  The window
 *            count is J[b] = h[b] + h[b + 1] for b in [-B, B], so J[B] = h[B].
 *   best   : the most J, then the most h[b], then the bin order above (smaller |b|, then the negative one).  No votes
 *            at all: bin 0 with 0 votes, as before.  By the second key a window whose lower bin is empty never wins
 *            (b + 1 covers the same votes and has h > 0), so the candidates are exactly the bins with votes; a row
 *            whose votes all lie in one bin reports that bin; with B = 0 the flag changes nothing.
 *   block  : best_bin holds b, the window's LOWER bin, and votes holds J[b] raw.  A hit now means stored = rate x
 *            upload + (best_bin + 0.5) x eps, within one eps.
 *   score  : v, u, the score (Jaccard, containment or local), min_votes, min_score, the exclusion, the order tuples
 *            and the block layouts take the new votes and best_bin and are otherwise as written for each call.
 *   rates  : per rate the best window by the rule above; the row keeps the rate with the most J, the smaller index on
 *            a tie.
 *   span   : P is the pairs that vote into b or into b + 1 - the latter only where b + 1 <= B -; t_first, t_last,
 *            c_lo, c_hi, nq and nr are defined over that P exactly as before, and TVZ_ALIGN_LOCAL scores from them.
 *   merges : tvz_align_{wide,rates,span}_topk_merge accept the bit and ignore it - the score is rebuilt from votes, nv
 *            and row_len, or from nq and nr, whichever way the votes were counted.  "All lists made with the same
 *            flags" covers this bit too.  _shards and _sharded pass it to the local call and to the merge.
 * No workspace size changes; the refusals keep their order and words; the flags are still checked where they were.
 * Cost: two more LDS reads per bin a row touches, no pass over the bins. */
#define TVZ_ALIGN_TWO_BINS 8u            /* flags: votes counted over two adjacent bins; best_bin = the lower one */
size_t tvz_align_wide_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k);
int tvz_align_wide_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                        int32_t max_query_len, double eps, double max_offset, int32_t min_votes, int32_t min_score,
                        uint32_t flags, const int32_t *d_exclude_ids, int32_t k, int32_t *d_out,
                        void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* The alignment top-k over a SHARDED table.  The block of tvz_align_topk is what travels: int32[Q][k+1][4], k rows
 * ascending in the order above, padding, then (-1, n_hits, 0, 0).  (TVZ_VERSION unchanged: new exports only.)
 *
 * tvz_align_topk_merge: d_gathered int32[n_lists][Q][k+1][4] (the shards' blocks, as an all-gather delivers them) ->
 * d_topk int32[Q][k][4], d_totals int32[Q].  A block row does not carry its order word: the score depends on nv, the
 * query's non-NaN count, which no block holds - so the merge takes the queries too, counts nv and rebuilds every
 * row's word with the expressions above.  Rules:
 *   - the k rows are the k smallest of the union by (word, row_len, votes); rows equal in all of that are identical
 *     rows and are all kept; fewer than k: padding rows (-1, 0, 0, 0) behind them;
 *   - a row with video_id < 0 is padding wherever it stands; so is a row whose u = nv + row_len - v would be 0
 *     (nv = 0 and row_len = 0: tvz_align_topk never writes one) - nothing divides by zero;
 *   - every list must be sorted as tvz_align_topk writes it (the merge stops reading a list at the first row that
 *     does not come before the k-th kept);
 *   - d_totals[q] = the lists' n_hits summed in 64 bits, clamped to INT32_MAX;
 *   - a query is REFUSED - all k rows padding, d_totals[q] = INT32_MIN - when any list's n_hits is negative (a shard
 *     refused it) or it is longer than 4,095 values.
 * n_lists outside 1..16 or k outside 1..64: TVZ_ERR_UNSUPPORTED; a NULL pointer, a negative Q, d_gathered or d_topk
 * not 16-byte aligned: TVZ_ERR_INVALID; nothing is written on a refusal; Q = 0 returns TVZ_OK.  Enqueues one launch.
 * Blocks of tvz_align_wide_topk are NOT this merge's: a best_bin outside +-2047 does not fit the word it rebuilds, and
 * the wide order is another one (tvz_align_wide_topk_merge takes them). */
int tvz_align_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, const double *d_queries,
                         const int64_t *d_q_offsets, int32_t *d_topk, int32_t *d_totals, void *hip_stream);
/* The shards of ONE process (several handles on one device, as tvz_match_topk_shards): tvz_align_topk on every handle
 * in turn on `hip_stream`, the blocks written to d_blocks int32[n_shards][Q][k+1][4], then tvz_align_topk_merge ->
 * d_topk, d_totals.  One workspace sized for ONE handle (tvz_align_topk_workspace_bytes) serves all of them.  Refuses
 * what tvz_align_topk and the merge refuse (n_shards outside 1..16 included) before anything is enqueued. */
int tvz_align_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                          const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps, double max_offset,
                          int32_t min_votes, int32_t min_score, const int32_t *d_exclude_ids, int32_t k,
                          int32_t *d_blocks, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                          size_t workspace_bytes, void *hip_stream);
/* One process per GPU: tvz_align_topk into the workspace's own block -> the ONE ncclAllGather of Q x (k+1) x 4 int32
 * per rank, ordered on the communicator with the other sharded calls' collectives -> tvz_align_topk_merge; every rank
 * gets the same d_topk int32[Q][k][4] and d_totals int32[Q].  Up to 16 ranks.
 * Workspace = tvz_align_topk_workspace_bytes(Q, max_query_len, total_query_keys, k)
 *           + (1 + max(n_ranks, 1)) x Q x (k + 1) x 16                                  (local + gathered blocks)
 *           + alignment (each part to 256 B).
 * Has run on hardware at ONE rank only. */
size_t tvz_align_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                              int32_t n_ranks);
int tvz_align_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                           int32_t Q, int32_t max_query_len, double eps, double max_offset, int32_t min_votes,
                           int32_t min_score, const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk,
                           int32_t *d_totals, void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* The alignment top-k AT ANY SHIFT over a SHARDED table: the three forms above for the block of tvz_align_wide_topk -
 * int32[Q][k+1][4], k rows (video_id, row_len, best_bin, votes) with best_bin anywhere in +-TVZ_ALIGN_WIDE_MAX_B,
 * ascending in the wide order of the call's `flags`, padding, then (-1, n_hits, 0, 0).  (TVZ_VERSION unchanged: new
 * exports only.)
 *
 * tvz_align_wide_topk_merge: d_gathered int32[n_lists][Q][k+1][4] -> d_topk int32[Q][k][4], d_totals int32[Q].  As
 * tvz_align_topk_merge it takes the queries, counts nv and rebuilds every row's score with the sweep's own
 * expressions: v = min(votes, nv, row_len); flags = 0: u = nv + row_len - v; flags & TVZ_ALIGN_CONTAIN: u = min(nv,
 * row_len); score = (v << 20) / u.  Rules:
 *   - the k rows are the k smallest of the union by the tuple (2^20 - score, video_id, best_bin as a signed number,
 *     row_len, votes); rows equal in all five are identical rows and are all kept; fewer than k: padding rows
 *     (-1, 0, 0, 0) behind them;
 *   - a row with video_id < 0 is padding wherever it stands; so is a row whose u is 0 under the call's score kind
 *     (with TVZ_ALIGN_CONTAIN any row with row_len = 0, and every row of a query with nv = 0) - nothing divides by
 *     zero;
 *   - PRECONDITION: every list is sorted as tvz_align_wide_topk writes it WITH THE SAME `flags` (the merge stops
 *     reading a list at the first row that does not come before the k-th kept); the two score kinds order
 *     differently, so blocks made with one must not be merged with the other;
 *   - d_totals[q] = the lists' n_hits summed in 64 bits, clamped to INT32_MAX;
 *   - a query is REFUSED - all k rows padding, d_totals[q] = INT32_MIN - when any list's n_hits is negative (a shard
 *     refused it) or it is longer than 4,095 values.
 * n_lists outside 1..16 or k outside 1..64: TVZ_ERR_UNSUPPORTED; a flag bit other than TVZ_ALIGN_CONTAIN, a NULL
 * pointer, a negative Q, d_gathered or d_topk not 16-byte aligned: TVZ_ERR_INVALID; nothing is written on a refusal;
 * Q = 0 returns TVZ_OK.  Enqueues one launch.  With flags = 0 and every best_bin within +-2047 the result equals
 * tvz_align_topk_merge's bit for bit. */
int tvz_align_wide_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                              const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk, int32_t *d_totals,
                              void *hip_stream);
/* The shards of ONE process (several handles on one device): tvz_align_wide_topk on every handle in turn on
 * `hip_stream`, the blocks written to d_blocks int32[n_shards][Q][k+1][4], then tvz_align_wide_topk_merge with the same
 * flags -> d_topk, d_totals.  One workspace sized for ONE handle (tvz_align_wide_topk_workspace_bytes) serves all of
 * them.  Refuses what tvz_align_wide_topk and the merge refuse (n_shards outside 1..16 included) before anything is
 * enqueued. */
int tvz_align_wide_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                               const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                               double max_offset, int32_t min_votes, int32_t min_score, uint32_t flags,
                               const int32_t *d_exclude_ids, int32_t k, int32_t *d_blocks, int32_t *d_topk,
                               int32_t *d_totals, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* One process per GPU: tvz_align_wide_topk into the workspace's own block -> the ONE ncclAllGather of Q x (k+1) x 4
 * int32 per rank, ordered on the communicator with the other sharded calls' collectives -> tvz_align_wide_topk_merge
 * with the same flags; every rank gets the same d_topk int32[Q][k][4] and d_totals int32[Q].  Up to 16 ranks; every
 * rank passes the same arguments.
 * Workspace = tvz_align_wide_topk_workspace_bytes(Q, max_query_len, total_query_keys, k)
 *           + (1 + max(n_ranks, 1)) x Q x (k + 1) x 16                                  (local + gathered blocks)
 *           + alignment (each part to 256 B).
 * Has run on hardware at ONE rank only. */
size_t tvz_align_wide_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                                   int32_t n_ranks);
int tvz_align_wide_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                int32_t Q, int32_t max_query_len, double eps, double max_offset, int32_t min_votes,
                                int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                                int32_t *d_topk, int32_t *d_totals, void *d_workspace, size_t workspace_bytes,
                                void *hip_stream);

/* The alignment top-k at any shift FOR SPEED-CHANGED COPIES: tvz_align_wide_topk with a list of rates, for the stored
 * video that is the upload played at another speed - film 24 -> 25 fps ("PAL speed-up", rate 24/25 or 25/24), the
 * 1000/1001 NTSC family, the "1.25x" re-upload.  There the cuts are c = rho x + t, and at a single rate the votes
 * smear over the bins.  (TVZ_VERSION unchanged: new exports only.)  The contract is tvz_align_wide_topk's, word for
 * word, with these changes:
 *   rates : h_rates is a HOST array of n_rates doubles, copied into the kernel's arguments - the call still only
 *           enqueues: no allocation, no host synchronisation.  n_rates outside 1..TVZ_ALIGN_MAX_RATES:
 *           TVZ_ERR_UNSUPPORTED; a NULL h_rates, or a rate that is NaN, infinite or <= 0: TVZ_ERR_INVALID; nothing is
 *           written on a refusal.  Equal rates may repeat.
 *   vote  : at rate i, x' = x * rho_i is ONE IEEE double multiplication rounded to nearest, and the pair (c, x) votes
 *           into floor((c - x')/eps + 0.5) when that lies in [-B, B].  The subtraction is NOT contracted with the
 *           product into an FMA.  B, its limits and its refusals are tvz_align_wide_topk's.
 *   best  : for each rate the best bin and its raw votes are found by the rule above (most votes, then smaller |bin|,
 *           then the negative one); the row keeps the rate with the MOST raw votes, on equal votes the SMALLER rate
 *           index - the caller lists rates by preference; no votes at any rate: rate index 0, bin 0.  Then v, u
 *           (Jaccard or TVZ_ALIGN_CONTAIN), score and the hit test are exactly as before; nv is the query's non-NaN
 *           count, whatever the rate.  A hit means: stored ~= rate x upload + best_bin x eps.
 *   order : ascending by the tuple (2^20 - score, video_id, best_bin as a signed number, row_len, votes, rate_index);
 *           rows equal in all six are identical rows and are all kept.
 *   d_out : int32[Q][k+1][5] = the k best rows as (video_id, row_len, best_bin, votes, rate_index), padding rows
 *           (-1, 0, 0, 0, 0), and a last row (-1, n_hits, 0, 0, 0); n_hits as the wide call's, INT32_MIN for a refused
 *           query included.  Rows are 20 bytes: nothing may assume a row is 16-byte aligned.
 * With n_rates = 1 and h_rates[0] = 1.0 (x * 1.0 == x) columns 0..3 of every row equal tvz_align_wide_topk's block bit
 * for bit, and column 4 is 0.
 * Workspace = tvz_match_tol_workspace_bytes(Q, max_query_len, max(total_query_keys, max_query_len))   (the sorted queries)
 *           + 4 Q                                                                      (hit totals)
 *           + max(6080, 95 Q) x k x 24                                                  (one kept list per sweep
 *             block; a kept hit is the wide call's two 64-bit words and 32-bit votes, and the 32-bit rate index)
 *           + alignment (each part to 256 B).
 * A workspace below the fixed parts + one query of max_query_len values: TVZ_ERR_WORKSPACE with the bytes missing.
 * Cost: a wave walks its row once per rate - n_rates times tvz_align_wide_topk's searches and votes - for ONE sort
 * of the queries, one read of the table's rows and one selection; and one hit per stored row at its best rate, which
 * no merge of per-rate calls can give (a block row does not say which table row it came from).
 *
 * tvz_align_rates_topk_merge: d_gathered int32[n_lists][Q][k+1][5] -> d_topk int32[Q][k][5], d_totals int32[Q]:
 * tvz_align_wide_topk_merge's rules with the six-tuple order.  The rate index is carried, never interpreted; the score
 * is rebuilt from votes, nv and row_len as there.  PRECONDITION: all lists were made with the same `flags` and the
 * same rate list.  Totals, refusals and limits (n_lists 1..16, k 1..64) as the wide merge; d_gathered and d_topk
 * 16-byte aligned (the base pointers only: the rows are not).
 * tvz_align_rates_topk_shards: the shards of ONE process (several handles on one device), as
 * tvz_align_wide_topk_shards: d_blocks int32[n_shards][Q][k+1][5]; one workspace sized for ONE handle
 * (tvz_align_rates_topk_workspace_bytes); refuses what tvz_align_rates_topk and the merge refuse before anything is
 * enqueued.
 * tvz_align_rates_topk_sharded: one process per GPU, as tvz_align_wide_topk_sharded relates to tvz_align_wide_topk:
 * the arguments of tvz_align_rates_topk with the communicator behind the handle; tvz_align_rates_topk into the
 * workspace's own block -> the ONE ncclAllGather of Q x (k+1) x 5 int32 per rank, ordered on the communicator with the
 * other sharded calls' collectives -> tvz_align_rates_topk_merge with the same flags; every rank gets the same d_topk
 * int32[Q][k][5] and d_totals int32[Q].  Every rank passes the same arguments, the rate list among them.  Refusals,
 * their order and their messages are tvz_align_rates_topk's; behind them, and still before anything is enqueued: a NULL
 * communicator, a NULL d_topk or d_totals, a d_topk that is not 16-byte aligned (TVZ_ERR_INVALID), more than 16 ranks
 * (TVZ_ERR_UNSUPPORTED).
 * Workspace = tvz_align_rates_topk_workspace_bytes(Q, max_query_len, total_query_keys, k)
 *           + (1 + max(n_ranks, 1)) x Q x (k + 1) x 20                                  (local + gathered blocks)
 *           + alignment (each part to 256 B);
 * tvz_align_rates_topk_sharded_workspace_bytes answers 0 where the plain sizing function does, and for n_ranks < 0.
 * Has run on hardware at ONE rank only. */
#define TVZ_ALIGN_MAX_RATES 8
size_t tvz_align_rates_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k);
int tvz_align_rates_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                         int32_t max_query_len, double eps, double max_offset, const double *h_rates, int32_t n_rates,
                         int32_t min_votes, int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                         int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream);
int tvz_align_rates_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                               const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk, int32_t *d_totals,
                               void *hip_stream);
int tvz_align_rates_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                                const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                                double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes,
                                int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                                int32_t *d_blocks, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                                size_t workspace_bytes, void *hip_stream);
size_t tvz_align_rates_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                                    int32_t n_ranks);
int tvz_align_rates_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                 int32_t Q, int32_t max_query_len, double eps, double max_offset, const double *h_rates,
                                 int32_t n_rates, int32_t min_votes, int32_t min_score, uint32_t flags,
                                 const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk, int32_t *d_totals,
                                 void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* The alignment top-k at any shift WITH THE MATCHED SPAN of every hit, and a score over that span alone:
 * tvz_align_rates_topk that also says WHERE the votes of the best bin lie - which part of the upload is the copy and
 * which part of the stored video was taken - for the excerpt from the middle and the clip inside a compilation.
 * (TVZ_VERSION unchanged: new exports only.)  The argument lists are those of the four tvz_align_rates_topk functions;
 * the call with the single rate 1.0 is tvz_align_wide_topk with spans.  The contract is tvz_align_rates_topk's, word
 * for word, with these changes:
 *   span  : for a row the rates contract has chosen (best_bin, rate_index), with rho = h_rates[rate_index]:
 *             s[0 .. nv) = the query's non-NaN values sorted ascending numerically;
 *             x'_t = s[t] * rho, ONE IEEE multiplication, not contracted with the subtraction;
 *             P = the pairs (row key c, index t) with floor((c - x'_t)/eps + 0.5) == best_bin - the vote's own
 *                 expression, never a rewrite; |P| is the raw `votes`;
 *             t_first = min t, t_last = max t over P;  nq = t_last - t_first + 1;
 *             c_lo, c_hi = the smallest and the largest key in P;  nr = #{keys c of the row : c_lo <= c <= c_hi}.
 *           Equal query values vote identically, -0.0 and +0.0 give the same difference, and infinities never vote:
 *           t_first and t_last do not depend on how the sort orders equal values.  A hit has votes >= 1, so P is not
 *           empty: 0 <= t_first <= t_last < nv, 1 <= nq <= nv, 1 <= nr <= row_len.
 *   flags : 0 and TVZ_ALIGN_CONTAIN mean what they mean in tvz_align_wide_topk.  TVZ_ALIGN_LOCAL: v = min(votes, nq,
 *           nr), u = nq + nr - v, score = (v << 20) / u - the Jaccard of the two sides INSIDE THE SPAN, in 0..2^20
 *           (v <= 4095, u >= v >= 1), exact integer arithmetic.  A 400-cut compilation that holds a 20-cut clip of a
 *           stored 400-cut film scores 20/780 by the Jaccard and 20/400 by the containment, and 2^20 here.  ONE vote
 *           gives nq = nr = 1 and the score 2^20: under TVZ_ALIGN_LOCAL min_votes is what keeps chance pairs out.
 *           TVZ_ALIGN_CONTAIN | TVZ_ALIGN_LOCAL (two score kinds) and any other bit: TVZ_ERR_INVALID.  The rate list
 *           and the flags are refused before the handle is looked at.  The other calls keep refusing bit 2.
 *   hit   : unchanged - v >= min_votes, score >= min_score, video_id != exclude_id - with v and score those of the
 *           call's score kind.
 *   order : ascending by the tuple (2^20 - score, video_id, best_bin as a signed number, row_len, votes, rate_index,
 *           t_first, t_last, nr); rows equal in all nine are identical rows and are all kept.
 *   d_out : int32[Q][k+1][8] = the k best rows as (video_id, row_len, best_bin, votes, rate_index, t_first, t_last,
 *           nr), padding rows (-1, 0, 0, 0, 0, 0, 0, 0), and a last row (-1, n_hits, 0, ...); n_hits = INT32_MIN for a
 *           refused query.  Rows are 32 bytes.
 * Without TVZ_ALIGN_LOCAL columns 0..4 of every row equal tvz_align_rates_topk's block bit for bit; with the single
 * rate 1.0, columns 0..3 equal tvz_align_wide_topk's.
 * Workspace = tvz_match_tol_workspace_bytes(Q, max_query_len, max(total_query_keys, max_query_len))   (the sorted queries)
 *           + 4 Q                                                                      (hit totals)
 *           + max(6080, 95 Q) x k x 32                                                  (one kept list per sweep
 *             block; a kept hit is the rates call's 24 bytes, ONE 32-bit word that holds t_first and t_last - 16 bits
 *             each, both below 4,095 - and the 32-bit nr)
 *           + alignment (each part to 256 B).
 * A workspace below the fixed parts + one query of max_query_len values: TVZ_ERR_WORKSPACE with the bytes missing.
 * Cost: tvz_align_rates_topk's, and for every row that passes min_votes and the exclusion - and, without
 * TVZ_ALIGN_LOCAL, min_score - one more walk of the row at the single best bin (about one window's visit) and one
 * pass over its keys that counts nr.
 *
 * tvz_align_span_topk_merge: d_gathered int32[n_lists][Q][k+1][8] -> d_topk int32[Q][k][8], d_totals int32[Q]:
 * tvz_align_rates_topk_merge's rules with the nine-tuple order.  Under flags 0 and TVZ_ALIGN_CONTAIN the score is
 * rebuilt from votes, nv and row_len as there; the three span columns are carried and take part in the order only.
 * Under TVZ_ALIGN_LOCAL the score is rebuilt from votes, nq = t_last - t_first + 1 and nr in 64-bit integer
 * arithmetic; a row with nq <= 0 or nr <= 0 is padding wherever it stands - nothing divides by zero.  Under every
 * flag a row whose t_first or t_last lies outside 0..4,094 (the call writes none) is padding too: the kept hit holds
 * 16 bits of each.  PRECONDITION: all lists were made with the same `flags` and the same rate list.  Totals, refusals
 * and limits (n_lists 1..16, k 1..64, d_gathered and d_topk 16-byte aligned) as the rates merge; the flags are
 * refused as the call refuses them.
 * tvz_align_span_topk_shards: the shards of ONE process, as tvz_align_rates_topk_shards: d_blocks
 * int32[n_shards][Q][k+1][8]; one workspace sized for ONE handle (tvz_align_span_topk_workspace_bytes).
 * tvz_align_span_topk_sharded: one process per GPU, as tvz_align_rates_topk_sharded: the ONE ncclAllGather moves Q x
 * (k+1) x 8 int32 per rank, the merge is tvz_align_span_topk_merge with the same flags; d_topk int32[Q][k][8].  Refusals
 * are tvz_align_span_topk's, in its order and words, and the communicator's behind them.
 * Workspace = tvz_align_span_topk_workspace_bytes(Q, max_query_len, total_query_keys, k)
 *           + (1 + max(n_ranks, 1)) x Q x (k + 1) x 32                                  (local + gathered blocks)
 *           + alignment (each part to 256 B).
 * Has run on hardware at ONE rank only. */
#define TVZ_ALIGN_LOCAL 2u               /* flags of tvz_align_span_topk: score = the Jaccard inside the span */
size_t tvz_align_span_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k);
int tvz_align_span_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                        int32_t max_query_len, double eps, double max_offset, const double *h_rates, int32_t n_rates,
                        int32_t min_votes, int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                        int32_t *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream);
int tvz_align_span_topk_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, uint32_t flags,
                              const double *d_queries, const int64_t *d_q_offsets, int32_t *d_topk, int32_t *d_totals,
                              void *hip_stream);
int tvz_align_span_topk_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries,
                               const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len, double eps,
                               double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes,
                               int32_t min_score, uint32_t flags, const int32_t *d_exclude_ids, int32_t k,
                               int32_t *d_blocks, int32_t *d_topk, int32_t *d_totals, void *d_workspace,
                               size_t workspace_bytes, void *hip_stream);
size_t tvz_align_span_topk_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                                   int32_t n_ranks);
int tvz_align_span_topk_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                                int32_t Q, int32_t max_query_len, double eps, double max_offset, const double *h_rates,
                                int32_t n_rates, int32_t min_votes, int32_t min_score, uint32_t flags,
                                const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk, int32_t *d_totals,
                                void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* EVERY ALIGNED PART of a named stored video: the refinement behind a search.  tvz_align_span_topk reports a stored
 * video once, at its single best shift; a re-upload with a part put in or taken out - an inserted ad, a removed
 * scene, two clips of one film - aligns at TWO shifts, and the search reports the larger half.  Given a batch of
 * uploads and, per upload, up to k stored video ids - out of a span block the search just wrote, an exact match, or a
 * pair a user reported - this call aligns each (upload, id) pair in full and reports up to TVZ_ALIGN_MAX_PARTS
 * disjoint parts.  Q x k row walks, not one per row of the table.  (TVZ_VERSION unchanged: new exports only.)
 *   ids    : the id of pair (q, j), 0 <= j < k, is d_video_ids[q * query_id_stride + j * id_stride]; the strides are in
 *            int32 units, so a span block int32[Q][k+1][8] is passed with strides (k+1)*8 and 8 and no copy.  A negative
 *            id (-1) is no pair.
 *   refused before the handle is looked at, with tvz_align_span_topk's rules, order and messages: the host rate list
 *            (1..TVZ_ALIGN_MAX_RATES rates, each finite and > 0), min_votes >= 1, k in 1..64, max_query_len <= 4,095;
 *            then max_parts outside 1..TVZ_ALIGN_MAX_PARTS (TVZ_ERR_UNSUPPORTED), then eps > 0, max_offset >= 0 and
 *            B = floor(max_offset/eps + 0.5) <= TVZ_ALIGN_WIDE_MAX_B.
 *   pair   : s[0 .. m) = the query's non-NaN values sorted ascending, x'_t = s[t] * rho (ONE IEEE multiplication, as in
 *            tvz_align_rates_topk); the pair (key c, index t) votes into floor((c - x'_t)/eps + 0.5).  The candidate
 *            rows are the rows of the table, as the alignment sweeps read it, whose video_id is the id; n_rows of them.
 *   part 0 of a row is tvz_align_span_topk's contract: per rate the best bin of [-B, B] (most votes; ties by the wide
 *            call's bin order), the rate with the most raw votes (the smaller index on a tie); P_0 = the pairs that
 *            vote into that bin at that rate, t_first / t_last the smallest / largest index and c_lo / c_hi the
 *            smallest / largest key over P_0; nq = t_last - t_first + 1, nr = the row's keys in [c_lo, c_hi].
 *   part i >= 1, at part 0's rate: the ALLOWED pairs have t outside every earlier part's [t_first, t_last] and c
 *            outside every earlier part's [c_lo, c_hi]; the best bin over them under the same tie rule; P_i, t_first,
 *            t_last, c_lo, c_hi from the allowed pairs at that bin; nq_i = the indices in [t_first_i, t_last_i] outside
 *            the earlier index ranges, nr_i = the row's keys in [c_lo_i, c_hi_i] outside the earlier key ranges.
 *   n_parts: a part is reported iff its raw votes are >= min_votes; the first part that fails ends the list, and so
 *            does max_parts.
 *   row    : among the rows that share the id, the one with the most part-0 votes; the earlier row of the table on a
 *            tie.  row_len and rate_index are that row's even when n_parts = 0.
 *   Equal query values vote identically, -0.0 and +0.0 give the same difference and infinities never vote: nothing
 *   depends on how the sort orders equal values.
 *   d_parts: int32[Q][k][1 + max_parts][6].  Row 0 = (video_id, row_len, rate_index, n_parts, n_rows, m); rows 1.. =
 *            (bin, votes, t_first, t_last, nq, nr), zeros beyond n_parts.  A negative id: (-1, 0, 0, 0, 0, m).  An id
 *            the table does not hold: (id, 0, 0, 0, 0, m).  n_parts = INT32_MIN marks a REFUSED pair, (id, 0, 0,
 *            INT32_MIN, n_rows, m): its query has more than max_query_len values (or more than 4,095; m reads 0 then),
 *            or more than TVZ_ALIGN_PARTS_MAX_ROWS rows share the id - n_rows still holds the true count.
 * The call only enqueues: no allocation, no host synchronisation; it takes the handle's shared lock and waits for the
 * mutations that have returned, as the other batched calls do.
 * Workspace = tvz_match_tol_workspace_bytes(Q, max_query_len, max(total_query_keys, max_query_len))   (the sorted queries)
 *           + Q k x 4                                     (rows per pair)
 *           + Q k x 8 x 8                                 (the candidate rows of a pair)
 *           + Q k x 8 x (1 + max_parts) x 24              (every candidate's parts)
 *           + alignment (each part to 256 B).
 * tvz_align_parts_workspace_bytes answers 0 for a negative size, k < 1 or max_parts outside 1..4.  A workspace below the
 * fixed parts + one query of max_query_len values: TVZ_ERR_WORKSPACE with the bytes missing.
 * Cost: one pass over the row table's 16-byte rows (a thread per row), then per (pair, candidate row) the span call's
 * walk of that one row and one more walk per further part.
 *
 * Over a SHARDED table every shard answers every pair and the answers are merged:
 * tvz_align_parts_merge: d_gathered int32[n_lists][Q][k][1 + max_parts][6], the lists' d_parts of ONE call (the same
 * queries, ids and parameters on every shard) -> d_parts int32[Q][k][1 + max_parts][6].  Per pair:
 *   - the lists whose n_rows > 0 are considered; among them the winner is the list with the most part-0 votes (row 1,
 *     column 1), the LOWER list index on a tie; where no list holds a row, list 0 is the winner;
 *   - the winner's block is copied, and n_rows becomes the lists' sum, accumulated in 64 bits and saturated at
 *     INT32_MAX;
 *   - if ANY list has n_parts = INT32_MIN the pair is REFUSED: rows 1.. become zero and row 0 becomes (the winner's id,
 *     0, 0, INT32_MIN, the summed n_rows, the winner's m);
 *   - ids are carried and never compared.
 * The rule is associative under regrouping: more than 16 lists are merged in groups of up to 16 and the groups' answers
 * merged again, lower lists first.  n_lists outside 1..16, k outside 1..64 or max_parts outside 1..TVZ_ALIGN_MAX_PARTS:
 * TVZ_ERR_UNSUPPORTED; a negative Q or a NULL pointer: TVZ_ERR_INVALID; nothing is written on a refusal; Q = 0 returns
 * TVZ_OK.  A pair's block is (1 + max_parts) x 24 bytes: the pointers need int32 alignment only.  Enqueues one launch.
 * MORE THAN TVZ_ALIGN_PARTS_MAX_ROWS ROWS of one id refuse a pair only where they lie in ONE shard: nine rows split five
 * and four over two shards are answered, with n_rows = 9; nine rows in one shard are refused, with n_rows = 9.
 * tvz_align_parts_shards: the shards of ONE process (several handles on one device): tvz_align_parts on every handle in
 * turn on `hip_stream` - each takes its handle's shared lock, waits for its mutations and selects its device -, the
 * answers written to d_blocks int32[n_shards][Q][k][1 + max_parts][6], then tvz_align_parts_merge -> d_parts.  One
 * workspace sized for ONE handle (tvz_align_parts_workspace_bytes) serves all of them.  Refuses what tvz_align_parts
 * refuses, in its order and words, then what the merge refuses (n_shards outside 1..16 included), a NULL handle and
 * handles on different devices, before anything is enqueued.
 * tvz_align_parts_sharded: one process per GPU: tvz_align_parts into the workspace's own block -> the ONE ncclAllGather
 * of Q x k x (1 + max_parts) x 6 int32 per rank, ordered on the communicator with the other sharded calls' collectives
 * -> tvz_align_parts_merge; every rank gets the same d_parts.  Every rank passes the same arguments, the ids among
 * them.  Refusals are tvz_align_parts's, in its order and words; behind them, before anything is enqueued: a NULL
 * communicator or d_parts (TVZ_ERR_INVALID), more than 16 ranks (TVZ_ERR_UNSUPPORTED).
 * Workspace = tvz_align_parts_workspace_bytes(Q, max_query_len, total_query_keys, k, max_parts)
 *           + (1 + max(n_ranks, 1)) x Q k x (1 + max_parts) x 24                        (local + gathered answers)
 *           + alignment (each part to 256 B);
 * tvz_align_parts_sharded_workspace_bytes answers 0 where tvz_align_parts_workspace_bytes does, and for n_ranks < 0.
 * Has run on hardware at ONE rank only. */
#define TVZ_ALIGN_MAX_PARTS 4
#define TVZ_ALIGN_PARTS_MAX_ROWS 8
size_t tvz_align_parts_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                       int32_t max_parts);
int tvz_align_parts(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q, int32_t max_query_len,
                    const int32_t *d_video_ids, int64_t id_stride, int64_t query_id_stride, int32_t k, double eps,
                    double max_offset, const double *h_rates, int32_t n_rates, int32_t min_votes, int32_t max_parts,
                    int32_t *d_parts, void *d_workspace, size_t workspace_bytes, void *hip_stream);
int tvz_align_parts_merge(const int32_t *d_gathered, int32_t n_lists, int32_t Q, int32_t k, int32_t max_parts,
                          int32_t *d_parts, void *hip_stream);
int tvz_align_parts_shards(tvz_corpus *const *shards, int32_t n_shards, const double *d_queries, const int64_t *d_q_offsets,
                           int32_t Q, int32_t max_query_len, const int32_t *d_video_ids, int64_t id_stride,
                           int64_t query_id_stride, int32_t k, double eps, double max_offset, const double *h_rates,
                           int32_t n_rates, int32_t min_votes, int32_t max_parts, int32_t *d_blocks, int32_t *d_parts,
                           void *d_workspace, size_t workspace_bytes, void *hip_stream);
size_t tvz_align_parts_sharded_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys, int32_t k,
                                               int32_t max_parts, int32_t n_ranks);
int tvz_align_parts_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                            int32_t max_query_len, const int32_t *d_video_ids, int64_t id_stride, int64_t query_id_stride,
                            int32_t k, double eps, double max_offset, const double *h_rates, int32_t n_rates,
                            int32_t min_votes, int32_t max_parts, int32_t *d_parts, void *d_workspace,
                            size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------
 * Opt-in TOLERANT duplicate match.  NOT the reference's verdict: db.py:79,85-91 match exact float64
 * values, and that stays the default everywhere (tolerance 0).  README.md:291 promises "0.1 second
 * precision"; a corpus that mixes containers or frame rates needs it: the same 30 fps video muxed with
 * time base 1/15360 and 1/1000 prints a different %.6g pts_time for two frames in three (<= 0.34 ms
 * apart), a 30 -> 25 fps conversion moves a cut by up to 33.3 ms.
 *
 * For query q (a multiset, in order) and corpus row r (a set of canonical keys: NaN dropped, -0.0
 * folded to +0.0):
 *   match(i, r) <=> q[i] is not NaN and exists key in r: key == q[i] or fabs(q[i] - key) <= tol
 *   count       =   #{ i : match(i, r) }   (query multiplicity counts; a row key may serve several q[i])
 *   kth         =   index i of the min_match-th matching query element (TVZ_KTH_NEVER if
 *                   count < min_match, -1 if min_match <= 0)           (as tvz_match)
 *   hit        <=>  count >= min_match and video_id != exclude_id
 * q[i] - key is ONE IEEE double subtraction rounded to nearest (no FMA, no rewrite to q >= key - tol,
 * no fast-math; f64 subnormals are not flushed), so a numpy restatement is bit-exact; the == term keeps
 * +-inf matching itself.  tol must be finite and >= 0: NaN, inf or a negative value return
 * TVZ_ERR_INVALID and write nothing.  tol = 0 IS the exact verdict (for finite doubles fl(a - b) == 0
 * exactly when a == b): ids, counts and kth then equal tvz_find_duplicates / tvz_match bit for bit.
 * At large tolerances unrelated long videos match by chance: at 0.1 s a 200-cut query meets about two
 * keys of a random 200-cut row of a 10-minute-to-2-hour corpus.  Pass ~1 ms for remuxes, half a frame
 * for frame-rate conversions.
 * Cost: one sweep of the row table and key arena per query (no index), each key searched in the
 * numerically sorted query (in LDS up to 8,192 timestamps, in device memory beyond).
 * ------------------------------------------------------------------------ */

/* host in / host out: the tolerant drop-in for db.find_duplicates (+ kth for the streaming loop).
 * Output rules of tvz_find_duplicates: results sorted by (video_id, count, kth), *n_out = the number of
 * hits (the true count when it exceeds cap; only cap are written), h_out_kth may be NULL, any query
 * length.  One launch (two for min_match > 5) + one stream synchronisation, the hits written into
 * pinned host memory of the handle; no device allocation for queries of up to 4,095 timestamps. */
int tvz_find_duplicates_tol(tvz_corpus *c, const double *h_query, int64_t n, double tol,
                            int32_t min_match, int32_t exclude_id, int64_t cap, int32_t *h_out_ids,
                            int32_t *h_out_counts, int32_t *h_out_kth, int64_t *n_out);
/* Scratch of tvz_match_tol: per query a count, and the sorted copy of every query (12 B per
 * timestamp).  total_query_keys = the length of d_queries (0: Q x max_query_len). */
size_t tvz_match_tol_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys);
/* Batched, device-resident; hit lists in tvz_match's layout (d_hits int32[Q][cap][3] of (video_id,
 * count, kth) in unspecified order, d_hits_n int32[Q] = hits found, may exceed cap), so tvz_topk /
 * tvz_topk_shard apply.  d_hits_n = INT32_MIN for a query longer than max_query_len (as tvz_match),
 * and for one whose sorted copy does not fit the workspace (size it with the batch's key count).
 * A workspace without room for the per-query counts returns TVZ_ERR_WORKSPACE and says how many
 * bytes are missing.  Enqueues only (no host synchronisation, no allocation). */
int tvz_match_tol(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                  int32_t max_query_len, double tol, int32_t min_match, const int32_t *d_exclude_ids,
                  int32_t cap, int32_t *d_hits, int32_t *d_hits_n, void *d_workspace,
                  size_t workspace_bytes, void *hip_stream);

/* The tolerant match with the per-shard top-k kept inside the sweep: no hit lists, no cap.  The match is the
 * tolerant contract above, word for word (tol finite and >= 0, else TVZ_ERR_INVALID and nothing written; tol = 0
 * is the exact verdict).  A hit is the sortable word kth << 44 | video_id << 12 | count of the index lookups; every
 * sweep block keeps its k smallest words on chip and writes them, with ONE atomic for its hit count, at its end;
 * a second kernel selects each query's k smallest.  Nothing in device memory grows with the number of hits.
 *   d_out : int32[Q][k+1][3], the block of tvz_match_topk (so tvz_topk_merge and the all-gather take it
 *           unchanged): the k best hits ascending by (kth, video_id, count), padded with (-1, 0, TVZ_KTH_NEVER),
 *           + a row (-1, n_hits, TVZ_KTH_NEVER).  The k rows are EXACT and n_hits is the true count however many
 *           rows hit; it is never negated.  n_hits = INT32_MIN (all rows padding) for a query longer than
 *           max_query_len or one whose sorted copy does not fit the workspace; 0 on an empty corpus.
 * TVZ_ERR_UNSUPPORTED, by name: min_match outside 1..5 (kth would need the fix-up pass over hit lists), k outside
 * 1..64, max_query_len > 4,095 (count must fit the word's 12 bits; the sorted query is always in LDS).  Use
 * tvz_match_tol + tvz_topk_shard for those.
 * Workspace = tvz_match_tol_workspace_bytes(Q, max_query_len, total_query_keys)       (the sorted queries)
 *           + 4 Q                                                                     (hit totals)
 *           + max(6080, 95 Q) x k x 8                                                  (one kept list per sweep block:
 *             the sweep runs min(rows / 16, 6080 / Q clamped to 95..2048) row blocks per query)
 *           + (1 + max(n_ranks, 1)) x Q x (k + 1) x 12                                 (local + gathered blocks)
 *           + alignment (each part to 256 B).  For Q >= 64 that is below what tvz_match_tol at cap = 4,096 +
 * tvz_topk_shard need (95 lists of k = 64 words + the total: under the Q x 4096 x 12 B of hit lists alone).  Too small: TVZ_ERR_WORKSPACE with the bytes missing.
 * Enqueues only (no host synchronisation, no allocation); rows upserted before the call are seen. */
size_t tvz_match_tol_topk_workspace_bytes(int32_t Q, int32_t max_query_len, int64_t total_query_keys,
                                          int32_t k, int32_t n_ranks);
int tvz_match_tol_topk(tvz_corpus *c, const double *d_queries, const int64_t *d_q_offsets, int32_t Q,
                       int32_t max_query_len, double tol, int32_t min_match, const int32_t *d_exclude_ids,
                       int32_t k, int32_t *d_out, void *d_workspace, size_t workspace_bytes,
                       void *hip_stream);
/* tvz_match_sharded for the tolerant match: tvz_match_tol_topk into the workspace's own block -> the ONE
 * ncclAllGather -> tvz_topk_merge.  d_topk int32[Q][k][3], d_totals int32[Q]: every block is exact, so a
 * total is the true hit count and is not negated for an overflow - there is none.  The one negative total left
 * is tvz_topk_merge's answer to a query some rank refused (n_hits = INT32_MIN in its block: longer than
 * max_query_len): the merge sums |n_hits| clamped to INT32_MAX and negates, as for any negative block total.  Workspace: the function above with the
 * communicator's n_ranks. */
int tvz_match_tol_sharded(tvz_corpus *c, tvz_comm *comm, const double *d_queries, const int64_t *d_q_offsets,
                          int32_t Q, int32_t max_query_len, double tol, int32_t min_match,
                          const int32_t *d_exclude_ids, int32_t k, int32_t *d_topk, int32_t *d_totals,
                          void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* Opt-in CELL POSTINGS for the batched tolerant calls, PER HANDLE (default off: a handle that never calls this
 * behaves and allocates exactly as before).  cell > 0: from now on every generation of the index - tvz_corpus_upload,
 * tvz_corpus_build_index, the background rebuild - also carries, per cell of `cell` seconds
 * (cell_of(x) = clamp(floor(x / cell), -2^40, +2^40): keys beyond +-2^40 cells, +-inf among them, share the two end
 * cells - slow there, still correct), the indexed rows that own a key in it, and the rows' 16-byte entries as they were
 * at the build's snapshot; a handle that already has an index builds one now (waits for matches in flight).  cell = 0:
 * off; the next build drops the postings.  cell must be 0 or finite and >= TVZ_TOL_CELL_MIN (x / cell then stays far
 * inside int64 for real timestamps); anything else returns TVZ_ERR_INVALID and changes nothing.
 * tvz_match_tol, tvz_match_tol_topk and tvz_match_tol_sharded then answer a batch from the postings near the queries'
 * timestamps instead of reading the whole corpus - every (query element, cell within tol) posting marks its row, rows
 * marked often enough are verified by the sweep's own row walk on the generation's row entry, the delta table is
 * swept as before - whenever tol <= cell, min_match is 1..5 and max_query_len <= 8,192 (list form) / 4,095 (top-k
 * form).  Every other call does what it did.  The contract above does not change by a bit: ids, counts, kth, totals
 * and top-k blocks equal those of a handle without postings (the hit lists of tvz_match_tol in a different,
 * unspecified, order); the workspace formulas still suffice.  tvz_find_duplicates_tol always sweeps.
 * For which tolerances it pays: where cell (>= tol) is small against the spacing of a video's cuts, so that few rows
 * own a key near a query's - at tol = cell = 1 ms on a 100k-row corpus a query of 200 timestamps verifies a few
 * thousand rows instead of reading 100,000 (profiles/tol_index.txt).  At 0.1 s most rows are candidates and the
 * lookup verifies nearly the whole corpus after paying for the postings: leave it off, or keep cell small and let
 * such calls sweep (tol > cell).  Cost: 2 B per (cell, row) posting + a directory + 16 B per row and generation, and a
 * second index build per rebuild. */
#define TVZ_TOL_CELL_MIN 9.5367431640625e-07 /* 2^-20 s */
int tvz_corpus_tol_index(tvz_corpus *c, double cell);
/* *cell = the cell width of the current generation's postings (0: none); out[0] = cells in use, out[1] = cell
 * postings, out[2] = builds so far that carried cell postings, out[3] = rows in the delta table the lookup shares
 * with the exact index.  out[0], out[1], out[3] are 0 while there are none.  cell / out may be NULL. */
int tvz_corpus_tol_index_stats(tvz_corpus *c, double *cell, int64_t out[4]);

/* ------------------------------------------------------------------------
 * Frame feeder I/O - the host side of what replaces the stderr pipe of
 * inspector/app.py:209-216: a micro-batch of luma planes from a file or a decoder pipe into the
 * caller's (pinned) buffer in one call, no per-frame host-language loop.
 * ------------------------------------------------------------------------ */

/* n_records fixed-size records from a seekable file (positioned reads: the descriptor's offset is not
 * used): record i starts at file_offset + i*record_bytes = [header_bytes header][payload_bytes payload]
 * [rest skipped].  YUV4MPEG2: header "FRAME\n", payload = the Y plane, rest = chroma.  `magic`
 * (nullable): header_bytes bytes every header must equal.  *n_done = whole records read (fewer at end
 * of file). */
int tvz_read_records(int fd, int64_t file_offset, int64_t n_records, int64_t record_bytes,
                     const void *magic, int64_t header_bytes, int64_t payload_bytes, void *h_dst,
                     int64_t *n_done);

/* The same from a pipe (`ffmpeg -f rawvideo -`): payload_bytes are kept, the following skip_bytes
 * (chroma planes) are read and dropped. */
int tvz_read_stream(int fd, int64_t n_records, int64_t payload_bytes, int64_t skip_bytes, void *h_dst,
                    int64_t *n_done);

#ifdef __cplusplus
}
#endif
#endif /* TVZ_H */
