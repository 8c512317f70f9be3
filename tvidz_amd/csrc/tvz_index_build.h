// tvz_index_build.h — the inverted index of a corpus handle: its build, synchronous and in the background (kernels:
// tvz_index_kernels.h, tvz_bucket_dir.h).  Included by tvz_match.hip only.
#pragma once
#include "tvz_handle.h"

namespace {

void index_drop(tvz_corpus *c) {
    Index &ix = c->ix;
    ix.valid = false;
    ix.n_delta = 0;
    ix.delta_slot.clear();
}

// The delta table holds delta_capacity() entries; a rebuild is started when it is HALF full, so
// upserts keep landing in the old generation's table while the new one is being built.
// A SMALL delta table: a build is ~1 ms per 20 M keys (9 ms for the unpartitioned build of a 1 M-row
// corpus) and runs in the background - a few microseconds of GPU per upsert at this trigger - while
// every batched match sweeps the whole delta table: 4096 queries against the 12,500 delta rows that
// max(4096, n / 8) allowed at 100k rows cost more than their lookup in the index of 100,000
// (profiles/r3_delta_probe.txt).
int64_t delta_trigger(int64_t n_main) { return std::max<int64_t>(kIndexMinDelta, n_main / 256); }
int64_t delta_capacity(int64_t n_main) { return 2 * delta_trigger(n_main) + 64; }

// Order `st` behind every match that has been enqueued so far: the event-tracked batched calls by
// a device-side wait (no host stall), the single-query sweeps in flight - not event-tracked, their
// callers are blocked in a stream synchronisation, ~20 us each - by waiting for them here.  Caller
// holds mu exclusively, so no new match can be enqueued meanwhile.
int stream_wait_readers(tvz_corpus *c, hipStream_t st) {
    {
        std::lock_guard<std::mutex> lk(c->ev_mu);
        for (int i = 0; i < tvz_corpus::kEvents; ++i)
            if (c->ev_pending[i]) TVZ_HIP(hipStreamWaitEvent(st, c->events[i].e, 0));
    }
    std::lock_guard<std::mutex> lk(c->stage_mu);
    for (Staging *s : c->all_staging)
        while (s->busy.load(std::memory_order_acquire)) std::this_thread::yield();
    return TVZ_OK;
}

// Host-side wait for the matches that still read index generation `gen` (the shadow about to be
// rebuilt: they were enqueued before the previous swap, i.e. thousands of upserts ago - this
// returns at once in practice).  Caller holds mu exclusively.
int wait_generation_idle(tvz_corpus *c, int gen) {
    {
        std::lock_guard<std::mutex> lk(c->ev_mu);
        for (int i = 0; i < tvz_corpus::kEvents; ++i)
            if (c->ev_pending[i] && c->ev_gen[i] == gen) {
                TVZ_HIP(hipEventSynchronize(c->events[i].e));
                c->ev_pending[i] = false;
            }
    }
    std::lock_guard<std::mutex> lk(c->stage_mu);
    for (Staging *s : c->all_staging)
        while (s->gen == gen && s->busy.load(std::memory_order_acquire)) std::this_thread::yield();
    return TVZ_OK;
}

// Wait for `st` without blocking inside the runtime: record an event and poll it.  A thread parked
// in hipStreamSynchronize for the length of a count pass (~1 ms) held up a lookup that called
// hipStreamSynchronize on ITS stream meanwhile (tests/rebuild_latency.c: one lookup per rebuild
// returned right when the builder's wait ended); a query of an event takes no such turn.
int wait_stream_polling(hipStream_t st, hipEvent_t ev) {
    TVZ_HIP(hipEventRecord(ev, st));
    while (true) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return TVZ_OK;
        if (e != hipErrorNotReady) return tvz::fail(TVZ_ERR_HIP, "index build failed: %s", hipGetErrorString(e));
        timespec nap = {0, 20 * 1000};
        nanosleep(&nap, nullptr);
    }
}

// The sizes of one generation's buffers and of the partitioned build's scratch, in elements, for a build of
// `live_keys` keys into a corpus reservation of rows_cap rows / keys_cap keys.  The build ensures them; build_index
// pre-sizes the shadow generation with them.
struct GenSizes {
    int64_t rows;     // ivid; the delta table holds delta_capacity(rows)
    int64_t pairs;    // (key, row) pairs: ix.pkeys / ix.prows
    // classic postings (+64: the lookup's last step reads up to 63 postings past the last list and discards them; x2 +
    // a line per size class and slice: the partitioned build pads keys to line-friendly places)
    int64_t post() const { return 2 * pairs + (int64_t)kIxMaxParts * kIxClasses * 64 + kIxPostPad; }
    int64_t ext16() const { return 2 * pairs + 64 * 1024; }      // external lists: whole lines, lists of > 40 postings only
    int64_t bucket_dir_bytes(uint32_t nb) const { return (int64_t)nb * kBkBytes + 2 * (ext16() + kIxPostPad); }
};

GenSizes gen_sizes(int64_t n_rows, int64_t live_keys, int64_t rows_cap, int64_t keys_cap) {
    return {std::max<int64_t>(rows_cap, n_rows), std::max<int64_t>(keys_cap, live_keys)};
}

// the classic directory of 2^log2 entries of `es` bytes, and the unpartitioned build's fill cursors for it
int64_t classic_dir_bytes(int log2, int es) { return ((int64_t)1 << log2) * es; }
int64_t fillc_words(int log2, int ks) { return ((int64_t)1 << log2) * (ks ? ks / 2 : 1); }

// The first half of the partitioned build, the same for both directory formats: every row's ivid entry, and the
// (key, row) pairs of rows [0, n_rows) grouped by directory slice in ix.pkeys / ix.prows; ix.pcnt holds the per-slice
// counts, then the slice starts (ix.pcnt.p + kIxMaxParts), then the scatter cursors.
int build_partition(tvz_corpus *c, const Row *d_rows, int64_t n_rows, int64_t live_keys, int64_t pairs, int bits,
                    int64_t n_parts, int32_t *ivid, hipStream_t st, double cellw = 0.0) {
    Index &ix = c->ix;
    if (int rc = ensure(ix.pkeys, pairs, 0)) return rc;
    if (int rc = ensure(ix.prows, pairs, 0)) return rc;
    if (int rc = ensure(ix.pcnt, 6 * (int64_t)kIxMaxParts + 8, 0)) return rc;
    uint32_t *cnt = ix.pcnt.p, *start = cnt + kIxMaxParts, *cur = start + kIxMaxParts + 1;
    // rows per block of the partition kernels: ~16 pairs per block and slice, so that a block's
    // one reservation per slice is a small share of its work
    const int64_t mean_len = std::max<int64_t>(1, live_keys / n_rows);
    const int32_t rpb = (int32_t)std::min<int64_t>(4096, std::max<int64_t>(kBlock / 64 * 2, 16 * n_parts / mean_len));
    hipLaunchKernelGGL(ix_part_clear_kernel, dim3(4), dim3(kBlock), 0, st, cnt, (int)n_parts, ix.info.p);
    hipLaunchKernelGGL(ix_partition_kernel, dim3((unsigned)tvz::ceil_div(n_rows, rpb)), dim3(kBlock), (size_t)n_parts * 4, st,
                       d_rows, n_rows, rpb, c->keys.p, bits, (int)n_parts, cnt, ivid, cellw);
    hipLaunchKernelGGL(ix_part_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, (int)n_parts, start, cur, ix.info.p);
    // the scatter: rows worth about one staging area per block
    const int32_t srpb = (int32_t)std::max<int64_t>(1, kIxStagePairs / mean_len);
    const size_t sclds = (size_t)kIxStagePairs * 12 + ((size_t)3 * n_parts + 1) * 4;
    hipLaunchKernelGGL(ix_scatter_kernel, dim3((unsigned)tvz::ceil_div(n_rows, srpb)), dim3(kIxScatterBlock), sclds,
                       st, d_rows, n_rows, srpb, c->keys.p, bits, (int)n_parts, cur, ix.pkeys.p, ix.prows.p, cellw);
    return TVZ_OK;
}

// the build's result, read back once its launches are done
int read_build_info(Index &ix, hipStream_t st, IxBuildInfo &info) {
    TVZ_HIP(hipGetLastError());
    TVZ_HIP(hipMemcpyAsync(ix.h_info.h, ix.info.p, sizeof(info), hipMemcpyDeviceToHost, st));
    if (int rc = wait_stream_polling(st, ix.build_ev.e)) return rc;
    info = *ix.h_info.h;
    return TVZ_OK;
}

// One sub-index: the bucket directory (tvz_bucket_dir.h).  Bytes the records need: 8 per distinct key + 2 per posting;
// buckets for a fill of kBkFillPct % of their payload.  Fuller: more lists do not fit beside their bucket's other
// records and move to the external area - a second line for every lookup that asks for them, and the long lists are
// the ones asked for most; emptier: a larger table.  The distinct keys are known from the last build, else guessed and
// the build repeated once at the size the count revealed.  Leaves d.nb = 0 when the keys do not fit (the classic
// format then).
int build_bucket_dir(tvz_corpus *c, IndexBuf &b, const Row *d_rows, int64_t n_rows, int64_t live_keys,
                     const GenSizes &sz, hipStream_t st, IxBuildInfo &info) {
    Index &ix = c->ix;
    Directory &d = b.keys;
    auto buckets_for = [&](double distinct) {
        const double bytes = 8.0 * distinct + 2.0 * (double)live_keys;
        const int64_t want = (int64_t)(bytes * 100.0 / ((double)kBkFillPct * kBkPayload)) + 1;
        return (uint32_t)std::min<int64_t>(tvz::round_up(std::max<int64_t>(want, kBkSlice), kBkSlice), (int64_t)kIxMaxParts * kBkSlice);
    };
    double distinct = ix.key_hint.post > 0 ? (double)ix.key_hint.distinct * (double)live_keys / (double)ix.key_hint.post * 1.1
                                           : (double)live_keys / 4.0;
    uint32_t nb = buckets_for(distinct);
    bool resized = false;
    for (int attempt = 0; attempt < 8; ++attempt) {
        const int64_t n_parts = nb / kBkSlice;
        if (int rc = build_partition(c, d_rows, n_rows, live_keys, sz.pairs, -(int)nb, n_parts, b.ivid.p, st)) return rc;
        if (int rc = ensure(d.dir, sz.bucket_dir_bytes(nb), 0)) return rc;
        hipLaunchKernelGGL(bk_slice_build_kernel, dim3((unsigned)n_parts), dim3(kBkBuildBlock), kBkBuildLds, st,
                           ix.pkeys.p, ix.prows.p, ix.pcnt.p + kIxMaxParts, d.dir.p, nb,
                           (uint32_t)std::min<int64_t>(sz.ext16(), 0x7fffffffLL), ix.info.p);
        if (int rc = read_build_info(ix, st, info)) return rc;
        if (!info.failed) {
            const uint32_t fit = buckets_for((double)info.n_distinct);
            // (a first build that guessed the distinct keys: once more at the right size if it is off by a quarter)
            if (!resized && (fit > nb + nb / 4 || fit + fit / 4 < nb)) { nb = fit; resized = true; continue; }
            d.nb = nb;
            d.ks = 0;
            d.log2 = 0;
            d.slice_log2 = 0;
            d.partitioned = false;
            return TVZ_OK;
        }
        if (nb >= (uint32_t)kIxMaxParts * kBkSlice) break;            // too many keys for slices of 256 buckets: classic format
        nb = (uint32_t)std::min<int64_t>(tvz::round_up((int64_t)nb + nb / 2, kBkSlice), (int64_t)kIxMaxParts * kBkSlice);
    }
    return TVZ_OK;
}

// The classic directory (tvz_index_kernels.h): ONE directory over the distinct keys of all rows, load <= 0.25
// (kIxDirLoadPct).  Sized from a guess - a fingerprint corpus repeats its keys many times over (cuts sit on frame
// grids) - and doubled while too crowded.
// Fills `d`, one of b's directories, sized from d's own `hint` or, the first time, for `guess` distinct keys if > 0.
// cellw > 0: the CELL directory of the tolerant lookup instead - the same build over cell ids (ix_build_key), the first
// time guessed from the key directory's distinct keys, an upper bound on the distinct cells - every key has one cell.
// Every (cell, row) pair is posted ONCE (ix_build_key drops a key whose cell is its arena predecessor's): the uint16
// counts per (cell, sub-index) rely on it.
int build_classic(tvz_corpus *c, IndexBuf &b, Directory &d, const DirHint &hint, int64_t guess, const Row *d_rows,
                  int64_t n_rows, int64_t live_keys, const GenSizes &sz, int n_sub, hipStream_t st, IxBuildInfo &info,
                  double cellw = 0.0) {
    Index &ix = c->ix;
    const int ks = ix_ks(n_sub), es = ix_entry_bytes(ks);
    const int64_t post_cap = sz.post();
    // the size for `distinct` keys: load <= kIxDirLoadPct - unless that directory is too large for the
    // partitioned build while one of half the size (load <= 0.5) is not (1 M rows x 62 sub-indexes: 144-byte
    // entries, 4,096 slices of 128 KB at load 0.5)
    auto partitionable = [&](int lg) {
        int sl = 6;
        while (((int64_t)2 << sl) * es <= kIxSliceBytes && sl < lg) ++sl;
        while ((((int64_t)1 << lg) >> sl) > kIxMaxParts && ((int64_t)2 << sl) * es <= kIxSliceBytesMax) ++sl;
        return (((int64_t)1 << lg) >> sl) <= kIxMaxParts && ((int64_t)es << sl) <= kIxSliceBytesMax;
    };
    auto size_for = [&](double distinct) {
        int lg = 10;
        while ((double)((int64_t)1 << lg) * kIxDirLoadPct < 100.0 * distinct && lg < 30) ++lg;
        if (!partitionable(lg) && partitionable(lg - 1) && (double)((int64_t)1 << (lg - 1)) >= 2.0 * distinct) --lg;
        return lg;
    };
    if (int rc = ensure(d.post, post_cap, 0)) return rc;
    int log2 = 10;
    if (hint.post > 0) {
        // the last build knows how often this corpus repeats its keys: one pass, no retry
        log2 = size_for((double)hint.distinct * (double)live_keys / (double)hint.post * 1.25);
    } else if (guess > 0) {
        log2 = size_for((double)guess);                // (the key directory of this snapshot was built a moment ago)
    } else {
        while (((int64_t)1 << log2) < live_keys / 8) ++log2;
    }
    // one row per wave and SHORT-LIVED blocks (no grid-stride loop): a background build shares the GPU
    // with lookups, whose few blocks get a CU as soon as any of these retires
    const int64_t blocks = tvz::ceil_div(n_rows, kBlock / 64);
    int slice_log2 = 0;
    bool shrunk = false, partitioned = false;
    while (true) {
        TVZ_REQUIRE(log2 <= 30, "index directory would exceed 2^30 entries");
        const int64_t dn = (int64_t)1 << log2;
        if (int rc = ensure(d.dir, classic_dir_bytes(log2, es), 0)) return rc;
        // Directory slices of ~32 KB (one block builds a slice in LDS; three such blocks leave room on
        // a CU for a lookup's block); larger ones if the slices would otherwise outnumber what the
        // partition kernels keep in LDS.  A directory of more than kIxMaxParts slices of 128 KB takes
        // the unpartitioned build (count + fill over the whole directory: one slice).
        slice_log2 = 6;
        while (((int64_t)2 << slice_log2) * es <= kIxSliceBytes && slice_log2 < log2) ++slice_log2;
        while ((dn >> slice_log2) > kIxMaxParts && ((int64_t)2 << slice_log2) * es <= kIxSliceBytesMax) ++slice_log2;
        const int64_t n_parts = dn >> slice_log2;
        partitioned = n_parts <= kIxMaxParts && post_cap < (int64_t)0xfffffff0LL &&   // (32-bit posting offsets)
                      ((int64_t)es << slice_log2) <= kIxSliceBytesMax;              // (entries of > 2 KB: > 16 M rows)
        if (!partitioned) slice_log2 = log2;
        const int bits = ix_dir_bits(log2, slice_log2);
        if (partitioned) {
            if (int rc = build_partition(c, d_rows, n_rows, live_keys, sz.pairs, bits, n_parts, b.ivid.p, st, cellw)) return rc;
            uint32_t *start = ix.pcnt.p + kIxMaxParts, *ptot = start + 2 * kIxMaxParts + 1, *pstart = ptot + kIxMaxParts;
            uint32_t *scratch = pstart + kIxMaxParts + 1;
            const size_t slds = std::max<size_t>(((size_t)es << slice_log2), (size_t)kIxSliceLdsFloor);
            hipLaunchKernelGGL(ix_slice_count_kernel, dim3((unsigned)n_parts), dim3(kIxSliceBlock), slds, st,
                               ix.pkeys.p, ix.prows.p, start, d.dir.p, es, ks, bits, ptot, ix.info.p);
            hipLaunchKernelGGL(ix_part_scan_kernel, dim3(1), dim3(1024), 0, st, ptot, (int)n_parts, pstart, scratch,
                               static_cast<IxBuildInfo *>(nullptr));
            hipLaunchKernelGGL(ix_slice_fill_kernel, dim3((unsigned)n_parts), dim3(kIxSliceBlock), slds, st,
                               ix.pkeys.p, ix.prows.p, start, pstart, d.dir.p, es, ks, bits, d.post.p);
        } else {
            const int64_t fillc = tvz::round_up(fillc_words(log2, ks), 4);
            if (int rc = ensure(ix.fillc, fillc, 0)) return rc;
            hipLaunchKernelGGL(ix_clear_kernel, dim3(2048), dim3(kBlock), 0, st, reinterpret_cast<uint4 *>(d.dir.p),
                               (size_t)(dn * es / 16), es / 16, reinterpret_cast<uint4 *>(ix.fillc.p),
                               (size_t)(fillc / 4), ix.info.p);
            hipLaunchKernelGGL(ix_count_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_rows, n_rows, c->keys.p,
                               d.dir.p, es, ks, bits, b.ivid.p, ix.info.p, cellw);
        }
        if (int rc = read_build_info(ix, st, info)) return rc;
        if (!info.failed && (int64_t)info.n_distinct * 2 <= dn) {            // accepted up to load 0.5; sized for kIxDirLoadPct
            // A directory guessed from the key count of a corpus that repeats its keys (the first
            // build of a handle) comes out many times too large - 4 M entries for 442 k distinct keys
            // at 100k rows, 128 MB instead of 32 - and at 1 M rows too large for the partitioned
            // build.  The count is cheap enough to run once more at the size it has just revealed
            // (load <= kIxDirLoadPct), if that is at least four times smaller.
            const int fit = size_for((double)info.n_distinct);
            if (!shrunk && (fit + 1 < log2 || fit > log2)) { log2 = fit; shrunk = true; continue; }   // (or too small for the target load)
            if (partitioned) break;
            hipLaunchKernelGGL(ix_offsets_kernel, dim3((unsigned)tvz::ceil_div(dn, kBlock)), dim3(kBlock), 0, st, d.dir.p,
                               (size_t)dn, es, ks, ix.info.p);
            hipLaunchKernelGGL(ix_fill_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_rows, n_rows, c->keys.p,
                               d.dir.p, es, ks, bits, ix.fillc.p, d.post.p, cellw);
            if (int rc = read_build_info(ix, st, info)) return rc;
            break;
        }
        ++log2;                                       // too crowded (or a slice overflowed): twice the directory
    }
    d.ks = ks;
    d.log2 = log2;
    d.slice_log2 = slice_log2;
    d.partitioned = partitioned;
    return TVZ_OK;
}

// Build the index of rows [0, n_rows) of the row table image `d_rows` (keys in c->keys) into
// generation `b` on stream `st`, and wait for it.  `b` must have no reader; nothing of the handle's
// published state is touched.  rows_cap / keys_cap: the corpus RESERVATION the buffers are sized
// with, so the rebuilds that upserts trigger allocate nothing until the corpus outgrows it.
// cellw > 0 (the handle's tvz_corpus_tol_index width, read under its lock by the caller): the generation also gets the
// cell postings and the rows' entries of this snapshot.
int build_kernels(tvz_corpus *c, IndexBuf &b, const Row *d_rows, int64_t n_rows, int64_t live_keys,
                  int64_t rows_cap, int64_t keys_cap, hipStream_t st, double cellw) {
    Index &ix = c->ix;
    // posting offsets and counts are 32-bit: a larger shard is swept (shard it over more GPUs)
    if (n_rows == 0 || live_keys >= (int64_t)0xfffffff0LL)
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "corpus of %lld rows / %lld keys gets no index", (long long)n_rows,
                         (long long)live_keys);
    const int n_sub = (int)tvz::ceil_div(n_rows, kSubRows);
    TVZ_REQUIRE(n_sub <= 4096, "too many rows for the index (%lld)", (long long)n_rows);
    const GenSizes sz = gen_sizes(n_rows, live_keys, rows_cap, keys_cap);
    if (int rc = ensure(b.ivid, sz.rows, 0)) return rc;
    if (int rc = ensure(b.drows, delta_capacity(sz.rows), 0)) return rc;
    IxBuildInfo info{};
    b.keys.nb = 0;
    if (n_sub == 1)
        if (int rc = build_bucket_dir(c, b, d_rows, n_rows, live_keys, sz, st, info)) return rc;
    if (b.keys.nb == 0)
        if (int rc = build_classic(c, b, b.keys, ix.key_hint, 0, d_rows, n_rows, live_keys, sz, n_sub, st, info)) return rc;
    if ((int64_t)info.cursor != live_keys)
        return tvz::fail(TVZ_ERR_INVALID, "internal: index holds %u postings for %lld keys", info.cursor,
                         (long long)live_keys);
    b.n_sub = n_sub;
    b.n_main = n_rows;
    b.keys.n_post = ix.key_hint.post = (int64_t)info.cursor;
    b.keys.n_distinct = ix.key_hint.distinct = (int64_t)info.n_distinct;
    b.n_spilled = info.n_spilled;
    b.n_ext = info.n_ext;
    b.max_spill = info.max_spill;
    b.ext_used = info.ext_cursor;
    b.t_cell = 0.0;
    b.cells.n_post = b.cells.n_distinct = 0;
    if (cellw > 0.0) {
        IxBuildInfo tinfo{};
        if (int rc = build_classic(c, b, b.cells, ix.cell_hint, ix.key_hint.distinct, d_rows, n_rows, live_keys, sz, n_sub,
                                   st, tinfo, cellw))
            return rc;
        if ((int64_t)tinfo.cursor > live_keys)         // (one posting per cell and row: at most one per key)
            return tvz::fail(TVZ_ERR_INVALID, "internal: cell index holds %u postings for %lld keys", tinfo.cursor,
                             (long long)live_keys);
        if (int rc = ensure(b.irows, sz.rows, 0)) return rc;
        TVZ_HIP(hipMemcpyAsync(b.irows.p, d_rows, (size_t)n_rows * sizeof(Row), hipMemcpyDeviceToDevice, st));
        if (int rc = wait_stream_polling(st, ix.build_ev.e)) return rc;
        b.t_cell = cellw;
        b.cells.n_post = ix.cell_hint.post = (int64_t)tinfo.cursor;
        b.cells.n_distinct = ix.cell_hint.distinct = (int64_t)tinfo.n_distinct;
    }
    if (b.keys.nb && tvz_debug())
        fprintf(stderr, "[tvz] bucket directory: %u buckets (%.1f MB) for %u keys / %u postings, fill %.2f, %u keys walked on "
                "(max %u buckets), %u external lists (%.1f MB)\n", b.keys.nb, b.keys.nb * 128e-6, info.n_distinct, info.cursor,
                (8.0 * info.n_distinct + 2.0 * info.cursor) / ((double)b.keys.nb * kBkPayload), info.n_spilled, info.max_spill,
                info.n_ext, info.ext_cursor * 2e-6);
    return TVZ_OK;
}

// Room in the shadow generation's directory `o` for a rebuild of the current one, `n`; `post` as large as n's: nothing
// for a bucket directory, whose postings live in `dir`.
void presize_directory(Index &ix, Directory &o, const Directory &n) {
    const int64_t dir_bytes = n.nb ? n.dir.cap / 2 : classic_dir_bytes(n.log2, ix_entry_bytes(n.ks));
    (void)ensure(o.dir, 2 * dir_bytes, 0);         // room for the directory to double once
    if (n.slice_log2 == n.log2)                    // the unpartitioned build's cursors
        (void)ensure(ix.fillc, 2 * fillc_words(n.log2, n.ks), 0);
    (void)ensure(o.post, n.post.cap, 0);
}

// Synchronous build of the whole row table (upload, explicit rebuild, after a compaction).  Caller
// holds mu exclusively, has drained every reader and no background build is running.
int build_index(tvz_corpus *c) {
    Index &ix = c->ix;
    index_drop(c);
    const int64_t n_rows = (int64_t)c->h_rows.size();
    if (n_rows == 0 || c->live_keys >= (int64_t)0xfffffff0LL) return TVZ_OK;
    IndexBuf &b = ix.buf[ix.cur ^ 1];
    if (int rc = build_kernels(c, b, c->rows.p, n_rows, c->live_keys, c->rows.cap, c->keys.cap, c->mstream.s, ix.tol_cell))
        return rc;
    ix.cur ^= 1;
    ix.valid = true;
    ++ix.builds;
    if (b.t_cell > 0.0) ++ix.tol_builds;
    // size the OTHER generation and the snapshot buffer now, while nobody is waiting: a background
    // rebuild then allocates nothing (hipMalloc / hipFree synchronise the whole device - a lookup in
    // flight would wait for them).
    IndexBuf &o = ix.buf[ix.cur ^ 1];
    const IndexBuf &n = ix.buf[ix.cur];
    const GenSizes sz = gen_sizes(n_rows, c->live_keys, c->rows.cap, c->keys.cap);
    presize_directory(ix, o.keys, n.keys);
    (void)ensure(o.ivid, n.ivid.cap, 0);
    (void)ensure(o.drows, n.drows.cap, 0);
    if (n.t_cell > 0.0) {                          // the cell postings' buffers, the same way
        presize_directory(ix, o.cells, n.cells);
        (void)ensure(o.irows, n.irows.cap, 0);
    }
    (void)ensure(ix.snap_rows, sz.rows, 0);
    (void)ensure(ix.dead_rows, n.drows.cap, 0);
    return TVZ_OK;
}

// No mutation that moves or frees the arena / row table / index buffers may run while a background
// build reads them: wait for it (the lock is released while waiting).
void wait_no_build(tvz_corpus *c, std::unique_lock<std::shared_mutex> &lk) {
    while (c->ix.building) c->ix.cv.wait(lk);
}

// Background rebuild, run by the upserting thread that crossed the threshold.  The handle's lock is
// RELEASED while the GPU builds: matches keep reading the current generation + its delta table,
// upserts keep landing there (and are logged in since_snap).  The build reads a stream-ordered
// snapshot of the row table and the append-only arena, fills the shadow generation on its own
// stream, and the swap - a few host operations plus one small copy and one small kernel on the
// mutation stream - publishes it.  Matches enqueued before the swap finish on the old generation,
// whose buffers stay untouched until the NEXT rebuild (which first waits for them).
int rebuild_in_background(tvz_corpus *c, std::unique_lock<std::shared_mutex> &lk) {
    Index &ix = c->ix;
    const double t_dbg0 = tvz_debug() ? tvz_now_us() : 0.0;
    const int64_t n_snap = (int64_t)c->h_rows.size();
    const int64_t live = c->live_keys, rows_cap = c->rows.cap, keys_cap = c->keys.cap;
    const double cellw = ix.tol_cell;
    const int shadow = ix.cur ^ 1;
    if (int rc = wait_generation_idle(c, shadow)) return rc;
    if (int rc = ensure(ix.snap_rows, std::max<int64_t>(rows_cap, n_snap), 0)) return rc;
    // the snapshot is ordered on the mutation stream: behind every upsert that has returned, ahead
    // of every later one
    TVZ_HIP(hipMemcpyAsync(ix.snap_rows.p, c->rows.p, (size_t)n_snap * sizeof(Row), hipMemcpyDeviceToDevice,
                           c->mstream.s));
    TVZ_HIP(hipEventRecord(ix.snap_ev.e, c->mstream.s));
    TVZ_HIP(hipStreamWaitEvent(ix.bstream.s, ix.snap_ev.e, 0));
    ix.building = true;
    ix.since_snap.clear();
    lk.unlock();
    const double t_dbg1 = tvz_debug() ? tvz_now_us() : 0.0;
    int rc = build_kernels(c, ix.buf[shadow], ix.snap_rows.p, n_snap, live, rows_cap, keys_cap, ix.bstream.s, cellw);
    char msg[512];
    if (rc) snprintf(msg, sizeof msg, "%s", tvz::err_buf());
    const double t_dbg2 = tvz_debug() ? tvz_now_us() : 0.0;
    lk.lock();
    if (tvz_debug())
        fprintf(stderr, "[tvz] rebuild: %lld rows, %lld keys, rc %d: locked prologue %.0f us, build (unlocked) %.0f us, "
                        "relock %.0f us, delta so far %lld\n", (long long)n_snap, (long long)live, rc, t_dbg1 - t_dbg0,
                t_dbg2 - t_dbg1, tvz_now_us() - t_dbg2, (long long)ix.since_snap.size());
    struct Done { Index &ix; ~Done() { ix.building = false; ix.since_snap.clear(); ix.cv.notify_all(); } } done{ix};
    if (rc) { snprintf(tvz::err_buf(), 512, "%s", msg); return rc; }
    IndexBuf &nb = ix.buf[shadow];
    // the new delta table: every row upserted since the snapshot, once, with its CURRENT entry
    std::vector<int64_t> &rs = ix.since_snap;
    std::sort(rs.begin(), rs.end());
    rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
    const int64_t d = (int64_t)rs.size();
    if (d > std::min<int64_t>(std::min(nb.drows.cap, ix.h_swap_cap), delta_capacity(nb.n_main)))
        return tvz::fail(TVZ_ERR_UNSUPPORTED, "%lld rows changed while the index was being rebuilt", (long long)d);
    if (d) {
        int64_t n_dead = 0;
        for (int64_t i = 0; i < d; ++i) {
            ix.h_swap_rows.h[i] = c->h_rows[(size_t)rs[(size_t)i]];
            if (rs[(size_t)i] < nb.n_main) ix.h_swap_dead.h[n_dead++] = (int32_t)rs[(size_t)i];
        }
        TVZ_HIP(hipMemcpyAsync(nb.drows.p, ix.h_swap_rows.h, (size_t)d * sizeof(Row), hipMemcpyHostToDevice, c->mstream.s));
        if (n_dead) {
            if (int rc2 = ensure(ix.dead_rows, n_dead, 0)) return rc2;
            TVZ_HIP(hipMemcpyAsync(ix.dead_rows.p, ix.h_swap_dead.h, (size_t)n_dead * 4, hipMemcpyHostToDevice, c->mstream.s));
            hipLaunchKernelGGL(ix_mark_dead_kernel, dim3((unsigned)tvz::ceil_div(n_dead, kBlock)),
                               dim3(kBlock), 0, c->mstream.s, nb.ivid.p, ix.dead_rows.p, (int32_t)n_dead);
            TVZ_HIP(hipGetLastError());
        }
        TVZ_HIP(hipEventRecord(c->mut_done.e, c->mstream.s));
        c->mut_any = true;
    }
    ix.delta_slot.clear();
    for (int64_t i = 0; i < d; ++i) ix.delta_slot.emplace(rs[(size_t)i], (int32_t)i);
    ix.n_delta = d;
    ix.cur = shadow;
    ix.valid = true;
    ++ix.builds;
    if (nb.t_cell > 0.0) ++ix.tol_builds;
    return TVZ_OK;
}

}  // namespace
