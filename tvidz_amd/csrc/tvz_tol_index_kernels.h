// tvz_tol_index_kernels.h — the tolerant match through CELL postings (tvz_corpus_tol_index), gfx950 wave64.
// Included by tvz_match.hip only.  From tvz_index_kernels.h: the directory format, tol_cell_of; from tvz_tol_kernels.h:
// tol_row_scan / tol_row_reduce, the top-k keeper; from tvz_match_kernels.h: the block's hit sink, kth_of.
//
// The sweeps of tvz_tol_kernels.h read every row to learn, almost always, that it has nothing near the query.  A
// generation of the index that carries cell postings knows, per cell of `w` seconds, the indexed rows that own a key in
// it (a classic directory over cell ids, postings ordered by sub-index of 2^14 rows - the exact index's format and
// build), and the 16-byte entry of every indexed row as it was at the build's snapshot.
//
// Probe range.  For query element q the cells [tol_cell_of(a), tol_cell_of(b)] are probed, with
//     a = fl(fl(q - tol) - m),   b = fl(fl(q + tol) + m),   m = w / 1024 (exact: a power-of-two scaling).
// Claim: every key with  key == q or fabs(fl(q - key)) <= tol  has  tol_cell_of(key)  inside, given tol <= w.
//   tol_cell_of is monotone (a correctly rounded division by w > 0, floor and clamp all are), so a <= key <= b is
//   enough wherever a and b are not clamped away.  Take the upper side, the lower one mirrors it.
//   * fl(key - q) <= tol and fl is monotone with fl(tol) = tol, so key - q < tol + ulp(tol) <= tol + 2^-52 w.
//   * b >= (q + tol + m) (1 - 2^-53)^2, so b >= q + tol + m - 2^-52 (|q| + tol + m).
//   * For |q| <= 2^41 w that error is below 2^-11 w + 2^-51 w, and m = 2^-10 w covers it and the 2^-52 w above: key <= b.
//   * For |q| > 2^41 w: a matching key has |key| >= |q| - tol - 2^-52 w > 2^40 w = L w and the sign of q, so it lies in
//     the end cell on q's side; b >= q (1 - 2^-52) (or a <= q (1 - 2^-52) for negative q) is beyond L w too, and the
//     other end of the range is at most (at least) that end cell by the clamp.  +-inf: a = b = q, the end cell, and
//     the == term's only partner is the same infinity, in that cell.
//   The range is short: (b - a) / w <= 2 + 2^-9 + rounding below 2^-11, so floor(b / w) - floor(a / w) <= 3: at most
//   FOUR cells per element (tests/test_tol_index_cpu.py checks claim and length on random and adversarial values).
//
// One block per (query, group of sub-indexes, part): per sub-index
//   pass A  thread t takes (element, cell) pairs of the sorted query in LDS: probes the cell's directory entry and sets,
//           for every posting of the cell in this sub-index, the row's bit in seen1 - or in seen2 if seen1 was set.
//           A row that reaches min_match >= 2 has two distinct matching elements, each with a posting of the row in its
//           range: the candidates are seen2 (seen1 for min_match 1).  A superset - cells straddle the tolerance;
//   rank    prefix popcounts of the candidate bitmap;
//   verify  candidate j (of this block's part) -> bitmap word by a search of the ranks, bit by selection; a 16-lane
//           group runs the sweeps' own row walk (tol_row_scan) on the GENERATION's row entry: count and kth are the
//           sweep's, bit for bit; rows replaced since the build (ivid < 0) are the delta sweep's;
//   emit    as the sweep of the same form: hits staged in LDS and appended (tvz_match_tol), or the k best words kept
//           per wave and written as one partial list with one atomic for the total (tvz_match_tol_topk).
// Nothing in device memory grows with candidates or hits.
#pragma once
#include "tvz_index_kernels.h"
#include "tvz_match_kernels.h"
#include "tvz_tol_kernels.h"
#include "tvz_wave.h"

namespace {

constexpr int kTolIxWords = kSubRows / 32;               // words per bitmap: a sub-index exactly
constexpr int kTolIxWpt = kTolIxWords / kTolBlock;       // bitmap words per thread (rank)
static_assert(kTolIxWpt >= 1 && kTolIxWpt * kTolBlock == kTolIxWords, "whole bitmap words per thread");
constexpr int kTolIxCells = 4;                           // cells per element the proof above allows
constexpr int kTolIxMaxGroups = 64;                      // blocks per query at most (the top-k form: one list each)
// static LDS of the two forms (bitmaps 4 KiB, ranks 1 KiB, the parked arguments and a few words; + the hit stage or
// the waves' lists): an upper bound, tests/test_tol_index_cpu.py holds the code objects against it
constexpr int kTolIxStaticLds = kTolIxWords * 10 + 256 + (kQ1Stage * 12 > kTolTopkWaves * 64 * 16 ? kQ1Stage * 12 : kTolTopkWaves * 64 * 16);

__device__ __forceinline__ void tol_probe_range(double q, double tol, double w, int64_t &c_lo, int64_t &c_hi) {
    const double m = w * 0x1p-10;
    c_lo = tol_cell_of((q - tol) - m, w);
    c_hi = tol_cell_of((q + tol) + m, w);
}

// What pass A, a candidate's first two loads and the output paths read, parked in LDS: as kernel arguments they would
// sit in scalar registers across the row walk, which needs every one of them (the compiler spilled 30 of them to
// vector lanes); read back from LDS they are vector registers for as long as they are used.
struct TolIxParked {
    const unsigned char *dir;
    const uint16_t *post;
    double cellw, tol;
    const int32_t *ivid;
    const Row *irows;
    const int64_t *keys;
    int32_t *hits, *hits_n;
    unsigned long long *part;
    int32_t dir_bits, ks, cap, n_lists;
    int32_t slots_at, excl;             // LDS offset of the kept directory slots (one per pass-A task); 0 = none kept
};
constexpr uint32_t kTolIxNoSlot = kIxNoSlot;       // a task's cell has no directory entry (or the task has no cell)
constexpr uint32_t kTolIxRedo = 0xfffffffeu;       // a task with cells beyond its first: not kept, probed again
// A block that walks several sub-indexes keeps every task's directory slot from its first pass A (4 B per task, 16 B
// per query timestamp) when that fits next to the sorted query: the later passes then read the entry straight away -
// no cell arithmetic, no probe sequence.  Queries too long for it probe again per sub-index; same results.
constexpr int kTolIxSlotKeys = 2048;
inline size_t tol_index_lds_bytes(int32_t lds_keys, bool keep_slots) {
    return tol_lds_bytes(lds_keys) + (keep_slots ? (size_t)lds_keys * kTolIxCells * 4 : 0);
}

// grid = (n_groups * split, Q).  Block bx walks sub-indexes [grp * spb, ..) with grp = bx / split and verifies the
// candidates j with j / 16 mod split == bx mod split.  Sorted queries as ts_match_tol_kernel takes them (always in LDS).
// TOPK: part = uint64[Q][n_lists][k], this block's list is number bx; totals[q] += its hits.
// else: hits = [Q][cap][3], hits_n[q] += (zeroed by ts_tol_sort_kernel; the delta sweep adds to the same count).
template <int MODE, bool TOPK>
__global__ __launch_bounds__(kTolBlock) void ts_tol_index_kernel(
    const unsigned char *__restrict__ dir, int dir_bits, int ks, const uint16_t *__restrict__ post,
    const int32_t *__restrict__ ivid, const Row *__restrict__ irows, int64_t n_indexed, int32_t n_sub, int32_t spb,
    int32_t split, double cellw, const int64_t *__restrict__ keys, const double *__restrict__ sv,
    const int32_t *__restrict__ sp, const int64_t *__restrict__ q_offsets, const int32_t *__restrict__ qm,
    int32_t lds_keys, double tol, int32_t min_match, const int32_t *__restrict__ exclude_ids, int32_t cap,
    int32_t *__restrict__ hits, int32_t *__restrict__ hits_n, int32_t k, unsigned long long *__restrict__ part,
    int32_t n_lists, int32_t keep_slots) {
    static_assert(MODE == kModeM2 || MODE == kModeTop5, "kth is known inside the walk for min_match 1..5");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_bm1[kTolIxWords], s_bm2[kTolIxWords];
    __shared__ uint16_t s_rank[kTolIxWords];
    __shared__ uint32_t s_ws[kTolBlock / 64];
    __shared__ TolIxParked s_arg;
    const int q = blockIdx.y;
    const int bx = blockIdx.x;
    const int64_t at = q_offsets[q] - q_offsets[0];
    const int32_t m = qm[q];
    if (m < 0 || m > lds_keys) {             // refused by the preparation
        if (!TOPK && threadIdx.x == 0 && bx == 0) hits_n[q] = INT32_MIN;
        return;                              // (TOPK: ts_tol_topk_reduce_kernel flags it)
    }
    const TolQuery lq = tol_query_to_lds(smem, lds_keys, sv, sp, at, m);
    const double *s = lq.s;
    const int32_t *pos = lq.pos;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int gl = threadIdx.x & (kGroup - 1);
    const int g = threadIdx.x / kGroup;
    TolTopkWave tw = {};
    if constexpr (TOPK) tw = tol_topk_open(wv, lane);
    for (int i = threadIdx.x; i < kTolIxWords; i += kTolBlock) { s_bm1[i] = 0; s_bm2[i] = 0; }
    if (threadIdx.x == 0) {
        if constexpr (!TOPK) hit_open();
        s_arg.dir = dir;
        s_arg.post = post;
        s_arg.cellw = cellw;
        s_arg.tol = tol;
        s_arg.ivid = ivid;
        s_arg.irows = irows;
        s_arg.keys = keys;
        s_arg.hits = hits;
        s_arg.hits_n = hits_n;
        s_arg.part = part;
        s_arg.n_lists = n_lists;
        s_arg.dir_bits = dir_bits;
        s_arg.ks = ks;
        s_arg.cap = cap;
        s_arg.slots_at = keep_slots ? ((lds_keys + 1) & ~1) * 12 : 0;     // behind the sorted query (tol_lds_bytes)
        s_arg.excl = exclude_ids ? exclude_ids[q] : -1;
    }
    if (keep_slots) {                        // nothing kept yet: the first pass A probes
        uint32_t *ts = reinterpret_cast<uint32_t *>(smem + ((lds_keys + 1) & ~1) * 12);
        for (int e = threadIdx.x; e < m * kTolIxCells; e += kTolBlock) ts[e] = kTolIxRedo;
    }
    __syncthreads();

    const int grp = bx / split, prt = bx - grp * split;
    const int sub_lo = grp * spb;
    const int sub_hi = sub_lo + spb < n_sub ? sub_lo + spb : n_sub;
    auto dest = [&] { return HitList{s_arg.hits, &s_arg.hits_n[blockIdx.y], blockIdx.y, s_arg.cap}; };

    for (int sub = sub_lo; sub < sub_hi; ++sub) {
        // ---- pass A ----
        const unsigned char *a_dir = s_arg.dir;
        const uint16_t *a_post = s_arg.post;
        const double a_w = s_arg.cellw, a_tol = s_arg.tol;
        const int a_ks = s_arg.ks, es = 16 + 2 * a_ks;
        const int dir_log2 = s_arg.dir_bits & 0xff;
        const uint32_t smask = (1u << (s_arg.dir_bits >> 8)) - 1u;      // probes wrap inside the directory slice
        uint32_t *tslot = s_arg.slots_at ? reinterpret_cast<uint32_t *>(smem + s_arg.slots_at) : nullptr;
        auto probe = [&](int64_t cell) -> uint32_t {             // the directory slot of a cell, kTolIxNoSlot if none
            int2 key;                                            // (a step loads the entry's key alone: the walk reads its head)
            return ix_probe(a_dir, es, dir_log2, smask, cell, key);
        };
        auto walk = [&](uint32_t slot) {                         // the entry's postings in this sub-index mark their rows
            if (slot == kTolIxNoSlot) return;
            const unsigned char *e = a_dir + (size_t)slot * es;
            const int4 h = *reinterpret_cast<const int4 *>(e);
            uint32_t p = (uint32_t)h.z, len = (uint32_t)h.w;
            if (a_ks) {
                const uint16_t *cn = reinterpret_cast<const uint16_t *>(e + 16);
                for (int t = 0; t < sub; ++t) p += cn[t];
                len = cn[sub];
            }
            for (uint32_t t = 0; t < len; ++t) ix_touch(s_bm1, s_bm2, min_match, a_post[p + t]);
        };
        for (int task = threadIdx.x; task < m * kTolIxCells; task += kTolBlock) {
            uint32_t slot0 = tslot ? tslot[task] : kTolIxRedo;
            if (slot0 == kTolIxRedo) {
                const int j = task & (kTolIxCells - 1);
                int64_t c_lo, c_hi;
                tol_probe_range(s[task / kTolIxCells], a_tol, a_w, c_lo, c_hi);
                slot0 = c_lo + j <= c_hi ? probe(c_lo + j) : kTolIxNoSlot;
                // the last task of an element takes whatever lies beyond the fourth cell: nothing, by the proof
                const bool more = j == kTolIxCells - 1 && c_lo + j < c_hi;
                if (more)
                    for (int64_t cell = c_lo + j + 1; cell <= c_hi; ++cell) walk(probe(cell));
                if (tslot) tslot[task] = more ? kTolIxRedo : slot0;
            }
            walk(slot0);
        }
        __syncthreads();
        // ---- rank: candidates before every bitmap word (thread t owns words t * kTolIxWpt ..) ----
        const uint32_t *cand = min_match >= 2 ? s_bm2 : s_bm1;
        uint32_t cw[kTolIxWpt], c = 0;
#pragma unroll
        for (int w = 0; w < kTolIxWpt; ++w) { cw[w] = cand[threadIdx.x * kTolIxWpt + w]; c += __popc(cw[w]); }
        const uint32_t incl = wave_scan_incl(c);
        if (lane == 63) s_ws[wv] = incl;
        __syncthreads();
        uint32_t before, n_cand;
        waves_sum<kTolBlock / 64>(s_ws, wv, before, n_cand);
        ix_rank_store(s_rank + threadIdx.x * kTolIxWpt, cw, before + incl - c);
        __syncthreads();
        // ---- verify + emit: group g of part prt takes candidates prt * 16 + g, + split * 16, ... ----
        const uint32_t row0 = (uint32_t)sub << kSubLog2, n_idx = (uint32_t)n_indexed;   // (rows are counted in 31 bits)
        for (uint32_t base = (uint32_t)(prt * kTolGroups + wv * (64 / kGroup)); base < n_cand;
             base += (uint32_t)(split * kTolGroups)) {       // wave-uniform: the wave compacts as one
            const uint32_t idx = base + (uint32_t)(g & (64 / kGroup - 1));
            const bool in = idx < n_cand;
            int lo = 0, hi = kTolIxWords;                    // the last word whose rank is <= idx: it holds candidate idx
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((uint32_t)s_rank[mid] <= idx) lo = mid; else hi = mid;
            }
            uint32_t word = cand[lo];
            for (uint32_t skip = in ? idx - (uint32_t)s_rank[lo] : 0u; skip; --skip) word &= word - 1u;
            const uint32_t r = row0 + (uint32_t)(lo * 32 + (word ? __ffs((int)word) - 1 : 0));
            const bool reach = in && r < n_idx;
            const int32_t vid = s_arg.ivid[reach ? r : row0];   // unconditional loads (row0 < n_indexed: the sub-index exists)
            const Row row = load_row(s_arg.irows + (reach ? r : row0));
            const bool live = reach && vid >= 0 && vid != s_arg.excl;   // replaced since the build / the query's own video
            uint32_t cnt, m1, m2, tk[kTop];
            const int64_t *rk = s_arg.keys + row.off;        // (a live row's first key also serves the lanes past its end)
            tol_row_scan<MODE>(rk, rk, live ? row.len : 0, s, pos, m, a_tol, gl, cnt, m1, m2, tk);
            const bool hit = live && (int64_t)cnt >= (int64_t)min_match;
            if (__ballot(hit) == 0ull) continue;
            tol_row_reduce<MODE>(m1, m2, tk);
            const int32_t kth = kth_of<MODE>(min_match, m1, m2, tk, r);
            const bool lead = hit && gl == 0;
            if constexpr (TOPK) tol_topk_offer(tw, lead, ix_tk_pack(kth, vid, cnt), k, lane);
            else if (lead) hit_emit<false>(vid, (int32_t)cnt, kth, HostOut{}, bx, dest);
        }
        __syncthreads();
        if (sub + 1 < sub_hi) {
            for (int i = threadIdx.x; i < kTolIxWords; i += kTolBlock) { s_bm1[i] = 0; s_bm2[i] = 0; }
            __syncthreads();
        }
    }
    // (the walk's last barrier is behind the last emit)
    if constexpr (TOPK) {
        tol_topk_finish(tw, k, wv, lane, [&] {
            return TolTopkOut{s_arg.part + ((int64_t)q * s_arg.n_lists + bx) * k, &s_arg.hits_n[q]};
        });
    } else {
        hit_flush<false, kTolBlock>(HostOut{}, bx, dest);
    }
}

}  // namespace
