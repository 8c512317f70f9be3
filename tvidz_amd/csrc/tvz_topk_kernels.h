// tvz_topk_kernels.h — the top-k family of the timestamp-corpus matcher (gfx950, wave64): the k best hits of a
// query's list(s) in (kth, video_id, count) order, and the merge of the per-rank blocks.
// Included by tvz_match_kernels.h, behind kBlock.
#pragma once
#include <climits>

#include "tvz_common.h"
#include "tvz_wave.h"

namespace {

// ---------------------------------------------------------------- forms, rows and totals
// What a launch reads and writes (a run-time argument, uniform over the launch).  A row is three int32
// (video_id, count, kth); a BLOCK is k + 1 rows per query: the k best, then the totals row (the layout of include/tvz.h).
//   plain  reads n_lists hit lists of `cap` rows per query (lists_n of them filled; all, if lists_n is NULL) and
//          writes topk[Q][k].
//   shard  reads one hit list per query and its counter lists_n[q * ns]; writes a block, so that one all-gather moves
//          rows and totals together.  Totals row: the true number of hits n, NEGATED when the list overflowed its
//          capacity (n > cap: the k best may then be inexact).
//   merge  reads n_lists gathered blocks [n_lists][Q][k + 1] (cap = k + 1) and writes topk[Q][k]; totals[q], unless
//          totals is NULL, is the sum of the blocks' |n|, negated if any of them was negative, so the caller knows to
//          run again with a larger capacity.
//   pair   reads two blocks like a merge (the index lookup's and the delta table's) and writes ONE block: its totals
//          row is the merge's total, also negated when the sum exceeds hit_cap - the one list an unfused match would
//          have filled.
enum TopkForm : int32_t { kTopkPlain = 0, kTopkShard = 1, kTopkMerge = 2, kTopkPair = 3 };
__host__ __device__ constexpr bool topk_writes_block(TopkForm f) { return f == kTopkShard || f == kTopkPair; }
__host__ __device__ constexpr bool topk_reads_blocks(TopkForm f) { return f >= kTopkMerge; }

constexpr int kSortCap = 2048;

__device__ __forceinline__ uint64_t sort_key(int32_t vid, int32_t kth) {
    return ((uint64_t)((uint32_t)kth + 1u) << 32) | (uint32_t)vid;   // NEVER + 1 wraps in unsigned
}

// a sort_key word and its count -> an output row; ~0 (no entry) -> padding
__device__ __forceinline__ void topk_store_row(int32_t *o, uint64_t key, int32_t cnt) {
    if (key == ~0ULL) {
        o[0] = -1; o[1] = 0; o[2] = TVZ_KTH_NEVER;
    } else {
        o[0] = (int32_t)(uint32_t)key;
        o[1] = cnt;
        o[2] = (int32_t)(uint32_t)(key >> 32) - 1;
    }
}
__device__ __forceinline__ void topk_store_totals(int32_t *o, int32_t t) {
    o[0] = -1; o[1] = t; o[2] = TVZ_KTH_NEVER;
}
// the totals rule: saturated at INT32_MAX; negative = some hit list was truncated (INT32_MIN stands for a negated 0)
__device__ __forceinline__ int32_t topk_total(long long sum, bool over) {
    const int32_t t = sum > 0x7fffffffLL ? 0x7fffffff : (int32_t)sum;
    return !over ? t : (t == 0) ? INT32_MIN : -t;
}

__device__ void bitonic_sort(uint64_t *key, int32_t *cnt, int n /* power of two */) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n / 2; i += blockDim.x) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = key[lo], b = key[hi];
                const int32_t ca = cnt[lo], cb = cnt[hi];
                const bool gt = (a > b) || (a == b && ca > cb);
                if (gt == up) {
                    key[lo] = b; key[hi] = a;
                    cnt[lo] = cb; cnt[hi] = ca;
                }
            }
        }
    }
    __syncthreads();
}

// the first `pos` entries sorted ascending by (key, count), the k best of them kept; block-uniform
__device__ __forceinline__ void sort_and_keep(uint64_t *key, int32_t *cnt, int &pos, int k) {
    int P = 2;
    while (P < pos) P <<= 1;
    for (int i = pos + threadIdx.x; i < P; i += kBlock) { key[i] = ~0ULL; cnt[i] = 0; }
    bitonic_sort(key, cnt, P);
    if (pos > k) pos = k;
}

// ---- the block kernel: bitonic k best over several lists, or over gathered blocks too long for one wave ----
// Launched in the plain and merge forms.
__global__ __launch_bounds__(kBlock) void ts_topk_kernel(const int32_t *__restrict__ lists,
                                                         const int32_t *__restrict__ lists_n,
                                                         int32_t n_lists, int32_t Q, int32_t cap,
                                                         int32_t k, int32_t *__restrict__ topk,
                                                         TopkForm form, int32_t *__restrict__ totals) {
    __shared__ uint64_t key[kSortCap];
    __shared__ int32_t cnt[kSortCap];
    for (int q = blockIdx.x; q < Q; q += gridDim.x) {
    int pos = 0;  // block-uniform fill level
    long long total = 0;
    bool overflow = false;
    for (int l = 0; l < n_lists; ++l) {
        int n = lists_n ? lists_n[(int64_t)l * Q + q] : cap;
        const int32_t *src = lists + ((int64_t)l * Q + q) * (int64_t)cap * 3;
        if (n > cap) n = cap;
        if (topk_reads_blocks(form)) {
            n = cap - 1;
            const int32_t t = src[(cap - 1) * 3 + 1];   // negative: that shard overflowed
            total += t < 0 ? -(long long)t : t;
            if (t < 0) overflow = true;
        }
        int j = 0;
        while (j < n) {
            int m = n - j;
            if (m > kSortCap - pos) m = kSortCap - pos;
            for (int i = threadIdx.x; i < m; i += kBlock) {
                const int32_t vid = src[(j + i) * 3 + 0];
                key[pos + i] = vid < 0 ? ~0ULL : sort_key(vid, src[(j + i) * 3 + 2]);
                cnt[pos + i] = src[(j + i) * 3 + 1];
            }
            pos += m;
            j += m;
            __syncthreads();
            if (pos == kSortCap) sort_and_keep(key, cnt, pos, k);
        }
    }
    __syncthreads();
    sort_and_keep(key, cnt, pos, k);
    if (threadIdx.x == 0 && topk_reads_blocks(form) && totals) totals[q] = topk_total(total, overflow);
    for (int i = threadIdx.x; i < k; i += kBlock)
        topk_store_row(topk + ((int64_t)q * k + i) * 3, (i < pos) ? key[i] : ~0ULL, cnt[i]);
    __syncthreads();
    }
}

// ---- per-query k best of a (long) hit list -------------------------------------------------
// Order: (kth, video_id, count) ascending.  A full bitonic sort of ~2,000 hits per query to keep
// 16 was most of the fixed cost of a sharded batch; instead a histogram of kth (LDS, 4098 bins)
// gives the smallest bin B whose prefix holds k hits, and only the hits in bins <= B (k plus the
// ties of one bin) are sorted.  Lists that are short anyway skip the histogram.
// Launched in the plain and shard forms.
constexpr int kSelBins = 4098;                // kth -1 .. 4095 exactly, everything above shares the last
constexpr int kSelMin = 64;                   // lists up to this long are sorted directly (a 512-entry bitonic
                                              // sort per query was 24 us per 1024 queries on a 1/8 shard)
constexpr int kSelSmallK = 256;               // k up to this: 1024 candidates held at once (12 KiB; with the
                                              // histogram 29 KiB per block - 5 blocks per CU instead of 3)

__device__ __forceinline__ int sel_bin(int32_t kth) {
    const uint32_t b = (uint32_t)kth + 1u;    // -1 -> 0, NEVER -> 0x80000000
    return b < (uint32_t)(kSelBins - 1) ? (int)b : kSelBins - 1;
}

template <int kSelCap>
__global__ __launch_bounds__(kBlock) void ts_topk_select_kernel(
    const int32_t *__restrict__ lists, const int32_t *__restrict__ lists_n, int32_t ns, int32_t Q,
    int32_t cap, int32_t k, int32_t *__restrict__ topk, TopkForm form, const int32_t *__restrict__ flags) {
    constexpr int kSelChunk = kSelCap / 2;
    static_assert(kSelChunk % kBlock == 0, "whole passes of the block");
    __shared__ uint64_t key[kSelCap];
    __shared__ int32_t cnt[kSelCap];
    __shared__ uint32_t hist[kSelBins];
    __shared__ uint32_t part[kBlock];
    __shared__ int32_t s_pos, s_bin;
    // flags != NULL: ts_topk_wave_kernel went first and flagged the queries it left to this kernel
    for (int q = blockIdx.x; q < Q; q += gridDim.x) {
    if (flags && flags[q] == 0) continue;
    const int32_t total = lists_n ? lists_n[(size_t)q * ns] : cap;
    const bool overflow = total > cap;
    const int n = total > cap ? cap : (total < 0 ? 0 : total);
    const int32_t *src = lists + (int64_t)q * cap * 3;
    int limit = kSelBins - 1;                 // keep hits whose bin is <= limit
    if (threadIdx.x == 0) s_pos = 0;
    if (n > kSelMin) {
        for (int i = threadIdx.x; i < kSelBins; i += kBlock) hist[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kBlock)
            if (src[i * 3] >= 0) atomicAdd(&hist[sel_bin(src[i * 3 + 2])], 1u);
        __syncthreads();
        constexpr int kPer = (kSelBins + kBlock - 1) / kBlock;      // bins per thread
        uint32_t s = 0;
        for (int b = threadIdx.x * kPer; b < (threadIdx.x + 1) * kPer && b < kSelBins; ++b) s += hist[b];
        part[threadIdx.x] = s;
        __syncthreads();
        // threshold bin = first bin whose inclusive prefix reaches k.  One wave: lane l owns the
        // partial sums of threads 4l..4l+3 (a serial walk by one thread was ~10 us of dependent LDS
        // reads per block - most of this kernel)
        if (threadIdx.x < 64) {
            const int l = threadIdx.x;
            const uint32_t p0 = part[4 * l], p1 = part[4 * l + 1], p2 = part[4 * l + 2], p3 = part[4 * l + 3];
            const uint32_t incl = wave_scan_incl(p0 + p1 + p2 + p3);
            const unsigned long long reach = __ballot(incl >= (uint32_t)k);
            const int owner = reach ? __ffsll((long long)reach) - 1 : 63;
            if (l == owner) {
                uint32_t cum = incl - (p0 + p1 + p2 + p3);
                int t = 4 * l;
                if (cum + p0 < (uint32_t)k) { cum += p0; ++t;
                    if (cum + p1 < (uint32_t)k) { cum += p1; ++t;
                        if (cum + p2 < (uint32_t)k) { cum += p2; ++t; } } }
                int b = t * kPer;
                while (b < kSelBins - 1 && cum + hist[b] < (uint32_t)k) cum += hist[b++];
                s_bin = b;
            }
        }
        __syncthreads();
        limit = s_bin;
    }
    int pos = 0;                              // block-uniform fill level
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += kSelChunk) {
        const int i = j0 + threadIdx.x;
#pragma unroll
        for (int u = 0; u < kSelChunk / kBlock; ++u) {
            const int ii = i + u * kBlock;
            if (ii < n && ii < j0 + kSelChunk) {
                const int32_t vid = src[ii * 3], kth = src[ii * 3 + 2];
                if (vid >= 0 && sel_bin(kth) <= limit) {
                    const int p = atomicAdd(&s_pos, 1);
                    key[p] = sort_key(vid, kth);
                    cnt[p] = src[ii * 3 + 1];
                }
            }
        }
        __syncthreads();
        pos = s_pos;
        if (pos > kSelCap - kSelChunk) {     // no room for another chunk: reduce to the k best
            sort_and_keep(key, cnt, pos, k);
            if (threadIdx.x == 0) s_pos = pos;
            __syncthreads();
        }
    }
    __syncthreads();
    pos = s_pos;
    sort_and_keep(key, cnt, pos, k);
    const int orows = topk_writes_block(form) ? k + 1 : k;
    if (topk_writes_block(form) && threadIdx.x == 0)
        topk_store_totals(topk + ((int64_t)q * orows + k) * 3, topk_total(total, overflow));
    for (int i = threadIdx.x; i < k; i += kBlock)
        topk_store_row(topk + ((int64_t)q * orows + i) * 3, (i < pos) ? key[i] : ~0ULL, cnt[i]);
    __syncthreads();
    }
}

// ---- top-k of SHORT inputs: one wave per query, no block barrier ---------------------------
// A 1/8 shard's hit list (~260 hits per query) and the merge of the gathered per-rank lists
// (n_ranks x k entries) are a few hundred entries; a 256-thread block each, with ~30 block barriers,
// spent 30 us + 15 us per 4096-query batch on them - a third of a sharded batch - and most of that
// is the launch rate of 4096 blocks and barrier latency, not work.  Here a wave takes a query of up
// to 1024 entries (4, 8 or 16 per lane, in registers): a histogram of kth in the wave's own LDS (two 16-bit
// bins per word) gives the threshold bin; the entries up to that bin - k plus the ties of one bin,
// normally a handful more than k - are compacted one per lane and sorted by a bitonic network over
// the lanes (more than 64 of them: k rounds of wave-minimum instead).  Same order and output rows
// as ts_topk_select_kernel / ts_topk_kernel.  A list of more than 1024 entries is FLAGGED and left
// to the block kernel, which follows with a small grid and takes only the flagged queries.
// Launched in the shard, merge and pair forms.
constexpr int kWsE = 16;
constexpr int kWsMax = 64 * kWsE;
constexpr int kWsK = 64;                                      // lane i writes output row i
constexpr int kWsPerLane = ((kSelBins + 1) / 2 + 63) / 64;   // 33 words (66 bins) per lane
constexpr int kWsWords = kWsPerLane * 64;
static_assert(kWsWords * 2 >= kSelBins && (kWsPerLane & 1) == 1, "bins covered; odd stride = no bank conflicts");

// the per-wave work for E entries per lane; a wave picks the smallest E that holds its list
template <int E>
__device__ __forceinline__ void wave_topk_body(
    uint32_t *h, const int lane, const int q, const int n, const int32_t total_row,
    const int32_t *__restrict__ lists, int32_t n_lists, int32_t Q, int32_t cap, int32_t k,
    int32_t *__restrict__ topk, TopkForm form, int32_t *__restrict__ totals, int32_t *__restrict__ flags,
    int32_t hit_cap) {
    uint64_t key[E];
    int32_t cnt[E];
    int bin[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        key[e] = ~0ULL;
        cnt[e] = 0;
        bin[e] = -1;                           // -1: no entry
        if (i < n) {
            const int32_t *src;
            if (topk_reads_blocks(form)) {
                const int l = i / (cap - 1), j = i - l * (cap - 1);
                src = lists + (((int64_t)l * Q + q) * cap + j) * 3;
            } else {
                src = lists + ((int64_t)q * cap + i) * 3;
            }
            const int32_t vid = src[0];
            if (vid >= 0) {
                key[e] = sort_key(vid, src[2]);
                cnt[e] = src[1];
                bin[e] = sel_bin(src[2]);
            }
        }
    }
#pragma unroll
    for (int w = 0; w < kWsPerLane; ++w) h[lane + 64 * w] = 0;
    wave_lds_fence();
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (bin[e] >= 0) atomicAdd(&h[bin[e] >> 1], 1u << ((bin[e] & 1) * 16));
    wave_lds_fence();
    // lane l owns words 33 l .. 33 l + 32 (bins 66 l .. 66 l + 65)
    uint32_t mine = 0;
#pragma unroll
    for (int w = 0; w < kWsPerLane; ++w) {
        const uint32_t v = h[lane * kWsPerLane + w];
        mine += (v & 0xffffu) + (v >> 16);
    }
    const uint32_t incl = wave_scan_incl(mine);
    const uint32_t tot = wave_total(incl);
    const uint32_t need = tot < (uint32_t)k ? tot : (uint32_t)k;
    int n_cand = 0;
    uint64_t mk = ~0ULL;
    int32_t mc = 0;
    bool fits = true;
    if (tot) {
        // threshold bin B: the first whose inclusive prefix reaches `need`; the owner lane walks its bins
        const unsigned long long reach = __ballot(incl >= need);
        const int owner = __ffsll((long long)reach) - 1;
        // the owner's 33 words are re-read one per lane (lane j: word j of the owner), a scan over the
        // lanes finds the bin (a serial walk by the owner alone was 500 of this kernel's 1,700 instructions)
        const uint32_t before = __shfl(incl - mine, owner);          // entries in the bins of lower lanes
        const uint32_t wv = lane < kWsPerLane ? h[owner * kWsPerLane + lane] : 0u;
        const uint32_t c0 = wv & 0xffffu, c1 = wv >> 16;
        const uint32_t wincl = wave_scan_incl(c0 + c1);
        const unsigned long long wreach = __ballot(before + wincl >= need);
        const int wl = __ffsll((long long)wreach) - 1;                // the word that holds bin B
        const uint32_t below = before + wincl - (c0 + c1);            // entries before that word (lane wl's view)
        const bool first = below + c0 >= need;                        // B is the word's low bin?
        const int B = __shfl(2 * (owner * kWsPerLane + lane) + (first ? 0 : 1), wl);
        const uint32_t upto = __shfl(below + c0 + (first ? 0u : c1), wl);
        fits = upto <= 64u;
        if (fits) {
            wave_lds_fence();                  // the histogram is dead: its first words become the candidate list
            uint64_t *ck = reinterpret_cast<uint64_t *>(h);          // [64] keys
            int32_t *cc = reinterpret_cast<int32_t *>(h + 128);      // [64] counts
            uint32_t base = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const bool is = bin[e] >= 0 && bin[e] <= B;
                const unsigned long long bal = __ballot(is);
                const uint32_t ofs = lanes_below(bal);
                if (is) { ck[base + ofs] = key[e]; cc[base + ofs] = cnt[e]; }
                base += (uint32_t)__popcll(bal);
            }
            wave_lds_fence();
            n_cand = (int)upto;
            if (lane < n_cand) { mk = ck[lane]; mc = cc[lane]; }
            // bitonic network over the 64 lanes, ascending by (key, count)
#pragma unroll
            for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    const uint64_t ok = __shfl_xor(mk, stride);
                    const int32_t oc = __shfl_xor(mc, stride);
                    const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);
                    const bool other_less = ok < mk || (ok == mk && oc < mc);
                    const bool other_more = ok > mk || (ok == mk && oc > mc);
                    if (keep_min ? other_less : other_more) { mk = ok; mc = oc; }
                }
            }
        }
    }
    if (flags && lane == 0) flags[q] = 0;
    if (!fits) {
        // more than 64 entries up to the threshold bin (a big tie: e.g. hundreds of true duplicates
        // with the same kth).  Rare, so simple: k rounds, each takes the minimum of what is left -
        // per-lane minimum, DPP butterfly inside the 16-lane rows, the four rows through scalar
        // registers - and removes exactly one copy of it.  Lane r keeps output row r.
        mk = ~0ULL;
        mc = 0;
        for (int r = 0; r < k; ++r) {
            uint64_t bk = key[0];
            int32_t bc = cnt[0];
#pragma unroll
            for (int e = 1; e < E; ++e)
                if (key[e] < bk || (key[e] == bk && cnt[e] < bc)) { bk = key[e]; bc = cnt[e]; }
            uint64_t wk = bk;
            int32_t wc = bc;
#define TVZ_MIN_STEP(CTRL)                                                               \
            {                                                                              \
                const uint64_t ok = dpp16_64<CTRL>(wk);                                    \
                const int32_t oc = (int32_t)dpp16<CTRL>((uint32_t)wc);                     \
                if (ok < wk || (ok == wk && oc < wc)) { wk = ok; wc = oc; }                \
            }
            TVZ_ROW16_BUTTERFLY(TVZ_MIN_STEP)
#undef TVZ_MIN_STEP
            uint64_t rk = ~0ULL;
            int32_t rc = 0;
#pragma unroll
            for (int row = 0; row < 4; ++row) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)wk, row * 16);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(wk >> 32), row * 16);
                const int32_t oc = __builtin_amdgcn_readlane(wc, row * 16);
                const uint64_t ok = ((uint64_t)hi << 32) | lo;
                if (row == 0 || ok < rk || (ok == rk && oc < rc)) { rk = ok; rc = oc; }
            }
            if (rk == ~0ULL) break;            // nothing left: the remaining rows are padding
            if (lane == r) { mk = rk; mc = rc; }
            const unsigned long long holders = __ballot(bk == rk && bc == rc);
            if (lane == __ffsll((long long)holders) - 1) {
                bool gone = false;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (!gone && key[e] == rk && cnt[e] == rc) { key[e] = ~0ULL; gone = true; }
            }
        }
    }
    const int orows = topk_writes_block(form) ? k + 1 : k;
    if (lane < k) topk_store_row(topk + ((int64_t)q * orows + lane) * 3, mk, mc);
    if (form == kTopkShard && lane == 0) topk_store_totals(topk + ((int64_t)q * orows + k) * 3, total_row);
    if ((form == kTopkMerge && totals) || form == kTopkPair) {
        long long sum = 0;
        bool over = false;
        for (int l = lane; l < n_lists; l += 64) {
            const int32_t t = lists[(((int64_t)l * Q + q) * cap + (cap - 1)) * 3 + 1];
            sum += t < 0 ? -(long long)t : t;
            over = over || t < 0;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        over = __ballot(over) != 0ULL || (form == kTopkPair && sum > (long long)hit_cap);
        if (lane == 0) {
            const int32_t t = topk_total(sum, over);
            if (form == kTopkPair) topk_store_totals(topk + ((int64_t)q * orows + k) * 3, t);
            else totals[q] = t;
        }
    }
}

__global__ __launch_bounds__(kBlock) void ts_topk_wave_kernel(
    const int32_t *__restrict__ lists, const int32_t *__restrict__ lists_n, int32_t ns, int32_t n_lists,
    int32_t Q, int32_t cap, int32_t k, int32_t *__restrict__ topk, TopkForm form,
    int32_t *__restrict__ totals, int32_t *__restrict__ flags, int32_t hit_cap) {
    __shared__ uint32_t s_hist[kBlock / 64][kWsWords];
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (q >= Q) return;                        // no block barrier below: waves are on their own
    uint32_t *h = s_hist[threadIdx.x >> 6];
    int n;                                     // entries to look at
    int32_t total_row = 0;                     // shard form: the list's hit count (negated on overflow)
    if (topk_reads_blocks(form)) {
        n = n_lists * (cap - 1);               // cap = k + 1 rows per gathered list, the last one = totals
    } else {
        const int32_t total = lists_n ? lists_n[(size_t)q * ns] : cap;
        n = total > cap ? cap : (total < 0 ? 0 : total);
        total_row = topk_total(total, total > cap);
    }
    if (n > kWsMax) {                          // the block kernel's (the host passes flags whenever this can happen)
        if (lane == 0) flags[q] = 1;
        return;
    }
    if (n <= 64 * 4)
        wave_topk_body<4>(h, lane, q, n, total_row, lists, n_lists, Q, cap, k, topk, form, totals, flags, hit_cap);
    else if (n <= 64 * 8)
        wave_topk_body<8>(h, lane, q, n, total_row, lists, n_lists, Q, cap, k, topk, form, totals, flags, hit_cap);
    else
        wave_topk_body<kWsE>(h, lane, q, n, total_row, lists, n_lists, Q, cap, k, topk, form, totals, flags, hit_cap);
}

// ---- merge of the gathered per-rank blocks when they are SORTED (they are: tvz_match_topk / tvz_topk_shard write
// their k rows in ascending (kth, video_id, count) order) and there are at most 16 of them ----------------------------
// The one-wave kernel above treats the R x k gathered entries as an unordered set (histogram, compaction, 64-lane
// bitonic network: ~720 VALU instructions per query) - 15 % of a sharded batch's instructions on a 1/8 shard, on the
// stream that shares the GPU with the next batch's lookup.  Sorted inputs need a k-way merge only: a group of G =
// 2^ceil(log2 R) lanes takes one query, lane r walks list r (staged in LDS, one private run per lane: no
// synchronisation), and each of the k steps min-reduces the G heads by a DPP butterfly inside the group; the winner
// writes output row t and moves to its next entry.  64 / G queries per wave: ~50 instructions per query at R = 8,
// a plain copy at R = 1.  Totals: |n| summed over the ranks, negated if any rank's list overflowed (topk_total).
// The merge form only, for at most kMsMaxLists blocks of at most kMsMaxK rows.
constexpr int kMsMaxLists = 16;                            // one DPP row per query
constexpr int kMsMaxK = 64;                                 // 64 runs of 3 k + 1 words: 48 KiB of LDS
template <int G>
__global__ __launch_bounds__(64) void ts_topk_merge_sorted_kernel(const int32_t *__restrict__ lists, int32_t n_lists,
                                                                  int32_t Q, int32_t k, int32_t *__restrict__ topk,
                                                                  int32_t *__restrict__ totals) {
    extern __shared__ int32_t s_lists[];                   // [64][3 k + 1] (the odd stride spreads the lanes over the banks)
    const int lane = threadIdx.x;
    const int q = (int)blockIdx.x * (64 / G) + lane / G;
    const int r = lane % G;
    const bool live = q < Q && r < n_lists;
    int32_t *mine = s_lists + (size_t)lane * (3 * k + 1);
    int32_t t_r = 0;
    if (live) {
        const int32_t *src = lists + (((int64_t)r * Q + q) * (k + 1)) * 3;
        t_r = src[3 * k + 1];
        // twelve loads in flight at a time (k is a run-time value: the plain loop was 3 k dependent round trips)
        int i = 0;
        for (; i + 12 <= 3 * k; i += 12) {
            int32_t v[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) v[j] = src[i + j];
#pragma unroll
            for (int j = 0; j < 12; ++j) mine[i + j] = v[j];
        }
        for (; i < 3 * k; ++i) mine[i] = src[i];
    }
    // hit totals over the ranks (each butterfly step adds two disjoint sets of lanes)
    unsigned long long sum = t_r < 0 ? (unsigned long long)(-(long long)t_r) : (unsigned long long)t_r;
    uint32_t over = t_r < 0 ? 1u : 0u;
#define TVZ_MS_SUM(C) { sum += dpp16_64<C>(sum); over |= dpp16<C>(over); }
    if (G >= 2) TVZ_MS_SUM(0xB1)
    if (G >= 4) TVZ_MS_SUM(0x4E)
    if (G >= 8) TVZ_MS_SUM(0x141)
    if (G >= 16) TVZ_MS_SUM(0x140)
#undef TVZ_MS_SUM
    if (q < Q && r == 0 && totals) totals[q] = topk_total((long long)sum, over != 0);
    // the k-way merge: heads compared as (kth + 1, video_id, count, rank) - the order of the top-k kernels, made
    // unique inside a group by the rank.  Two 64-bit words per head and bitwise logic on the comparisons: the
    // short-circuit form compiled to a ladder of branches per butterfly step (and a lambda that captured the head
    // by reference put it in scratch memory: two scratch loads per output row).
    int p = 0;
    unsigned long long ha, hb;                                 // (kth + 1) << 32 | video_id ; count << 32 | rank
#define TVZ_MS_HEAD() do { \
        const int pp = p < k ? p : k - 1; \
        const int32_t v0 = mine[3 * pp], v1 = mine[3 * pp + 1], v2 = mine[3 * pp + 2]; \
        const bool ok = live & (p < k) & (v0 >= 0);            /* exhausted, or padding: the rest of a sorted list is padding too */ \
        ha = ok ? ((unsigned long long)((uint32_t)v2 + 1u) << 32) | (uint32_t)v0 : ~0ULL; \
        hb = ok ? ((unsigned long long)(uint32_t)v1 << 32) | (uint32_t)r : ~0ULL; \
    } while (0)
    TVZ_MS_HEAD();
    for (int t = 0; t < k; ++t) {
        unsigned long long ma = ha, mb = hb;
#define TVZ_MS_MIN(C) { const unsigned long long oa = dpp16_64<C>(ma), ob = dpp16_64<C>(mb); \
                        const bool lt = (oa < ma) | ((oa == ma) & (ob < mb)); \
                        ma = lt ? oa : ma; mb = lt ? ob : mb; }
        if (G >= 2) TVZ_MS_MIN(0xB1)
        if (G >= 4) TVZ_MS_MIN(0x4E)
        if (G >= 8) TVZ_MS_MIN(0x141)
        if (G >= 16) TVZ_MS_MIN(0x140)
#undef TVZ_MS_MIN
        if (q < Q) {
            int32_t *o = topk + ((int64_t)q * k + t) * 3;
            if (ma == ~0ULL) {                                 // every list is exhausted: padding from here on
                if (r == 0) { o[0] = -1; o[1] = 0; o[2] = TVZ_KTH_NEVER; }
            } else if ((uint32_t)mb == (uint32_t)r) {          // this lane's head is the smallest
                o[0] = (int32_t)(uint32_t)ma; o[1] = (int32_t)(mb >> 32); o[2] = (int32_t)((uint32_t)(ma >> 32) - 1u);
                ++p;
                TVZ_MS_HEAD();
            }
        }
    }
#undef TVZ_MS_HEAD
}

}  // namespace
