// tvz_gap_codes.h — the gap codes of one stored row, made on the host (include/tvz_gap.h: STORED SIDE), and the
// workspace layout of tvz_align_candidates and its form with rates, with the sharded form's front.  Plain C++ with no HIP in it:
// tvz_match.hip includes it for the handle, a stand-alone host program can include it on its own.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tvz_gap {

constexpr int kBinBits = 17;
constexpr double kMaxBin = 131071.0;                    // 2^17 - 1
constexpr double kBin1 = 131072.0;                      // 2^17
constexpr double kBin2 = 17179869184.0;                 // 2^34
constexpr int kVariants = 8;                            // probe slots of a query position
constexpr int kMaxProbes = 4095;                        // probe slots of a query (the lookup's longest query)
constexpr int kMaxC = 64;

// a bin is valid iff it lies in [0, kMaxBin]: compared on the double, NaN fails
inline bool bin_valid(double b) { return b >= 0.0 && b <= kMaxBin; }

// r_i of the contract: one subtraction, one true division
inline double gap_ratio(double lo, double hi, double gap_eps) {
    const double d = hi - lo;
    return d / gap_eps;
}

// the code of three valid bins: exact in a double (below 2^51)
inline double code_of(double g0, double g1, double g2) { return g0 + g1 * kBin1 + g2 * kBin2; }

// The codes of a row of `len` keys, appended to `out` in position order (duplicates are left in: the table that stores
// them keeps a row as a set).  `keys` are the handle's canonical bit patterns of float64 values: distinct, no NaN, -0.0
// folded - but sorted as INTEGERS, which puts negative values in descending order, so they are sorted numerically here
// first (`vals`: the caller's scratch, it keeps its capacity).  Returns how many codes were appended.
inline int64_t row_codes(const int64_t *keys, int64_t len, double gap_eps, std::vector<double> &vals, std::vector<double> &out) {
    if (len < 4) return 0;
    vals.resize((size_t)len);
    bool negative = false;
    for (int64_t i = 0; i < len; ++i) {
        memcpy(&vals[(size_t)i], &keys[i], 8);
        negative = negative || keys[i] < 0;
    }
    if (negative) std::sort(vals.begin(), vals.end());
    const size_t before = out.size();
    double b0 = std::floor(gap_ratio(vals[0], vals[1], gap_eps) + 0.5);
    double b1 = std::floor(gap_ratio(vals[1], vals[2], gap_eps) + 0.5);
    for (int64_t i = 0; i + 3 < len; ++i) {
        const double b2 = std::floor(gap_ratio(vals[(size_t)i + 2], vals[(size_t)i + 3], gap_eps) + 0.5);
        if (bin_valid(b0) && bin_valid(b1) && bin_valid(b2)) out.push_back(code_of(b0, b1, b2));
        b0 = b1;
        b1 = b2;
    }
    return (int64_t)(out.size() - before);
}

// ---- the workspace of tvz_align_candidates and tvz_align_candidates_rates (include/tvz_gap_rates.h) ----
// Regions of 256-byte multiples behind a base aligned up to 256 (the carver of tvz_match.hip walks the same sizes).
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// probe slots of a query of m sorted values; -1: the query is refused (m < 0: longer than max_query_len).  constexpr:
// the kernels call it too
constexpr int32_t probe_slots(int32_t m) {
    if (m < 0) return -1;
    if (m < 4) return 0;
    const int64_t s = (int64_t)kVariants * (m - 3);
    return s > kMaxProbes ? -1 : (int32_t)s;
}

// the longest probe list of a call whose queries have up to max_query_len values (at least one position's worth, so
// that the lookup never sees a zero length with a non-NULL query array)
inline int32_t max_probe_len(int32_t max_query_len) {
    const int64_t s = (int64_t)kVariants * std::max(max_query_len - 3, 1);
    return (int32_t)std::min<int64_t>(s, kMaxProbes / kVariants * kVariants);
}

// The lookup sees Q * R probe lists, R per query (list q * R + i is query q at rate i; the plain call: R = 1).  Per list:
// its hit list and count, its probe offset and - `with_excl`, the call with a rate list - its query's exclusion id; then
// the lookup's own workspace (`match_bytes`: its sizing function's answer for that many lists) and the Q queries'
// counts; then, for `room` query values - the call takes what the caller's buffer holds, at least one longest query -
// the sorted values, their positions and 8 probe slots per value and rate.  The queries the sort accepts lie in
// disjoint ranges of [0, room), so their probes never exceed 8 * R * room slots.
struct WsRegions {                   // byte offsets from the aligned base; excl is empty (= match) without with_excl
    size_t hits, hits_n, p_off, excl, match, qm, sv, sp, probes, end;
};
constexpr size_t per_key(int32_t R) { return sizeof(double) + sizeof(int32_t) + (size_t)R * kVariants * sizeof(double); }
constexpr size_t kWsSlack = 256 + 3 * 255;              // a line for the base, the roundings of the three sized regions

inline WsRegions ws_regions(int32_t Q, int32_t R, bool with_excl, int32_t cap, size_t match_bytes, int64_t room) {
    WsRegions r;
    const size_t lists = (size_t)Q * (size_t)R;
    size_t p = 0;
    r.hits = p;    p += al256(lists * (size_t)cap * 3 * sizeof(int32_t));
    r.hits_n = p;  p += al256(lists * sizeof(int32_t));
    r.p_off = p;   p += al256((lists + 1) * sizeof(int64_t));
    r.excl = p;    p += with_excl ? al256(lists * sizeof(int32_t)) : 0;
    r.match = p;   p += al256(match_bytes);
    r.qm = p;      p += al256((size_t)Q * sizeof(int32_t));
    r.sv = p;      p += al256((size_t)room * sizeof(double));
    r.sp = p;      p += al256((size_t)room * sizeof(int32_t));
    r.probes = p;  p += al256((size_t)room * (size_t)R * kVariants * sizeof(double));
    r.end = p;
    return r;
}
// bytes for `keys` query values; the most values a buffer of `bytes` holds (-1: not even the fixed parts) -
// ws_room(.., ws_bytes(.., keys)) is `keys`, and the regions of that room end inside the buffer at any base
inline size_t ws_bytes(int32_t Q, int32_t R, bool with_excl, int32_t cap, size_t match_bytes, int64_t keys) {
    return ws_regions(Q, R, with_excl, cap, match_bytes, 0).end + kWsSlack + (size_t)keys * per_key(R);
}
inline int64_t ws_room(int32_t Q, int32_t R, bool with_excl, int32_t cap, size_t match_bytes, size_t bytes) {
    const size_t fixed = ws_bytes(Q, R, with_excl, cap, match_bytes, 0);
    return bytes < fixed ? -1 : (int64_t)((bytes - fixed) / per_key(R));
}

// ---- tvz_align_candidates_long (include/tvz_gap_long.h): the segments of a long query and its workspace ----
// The positions 0 .. m - 4 of a query are cut into segments of kLongSegPositions consecutive positions, a probe list
// each: 8 x 511 = 4,088 slots, the most whole positions the lookup's longest query (kMaxProbes) holds.  constexpr: the
// kernels call them too.
constexpr int kLongSegPositions = kMaxProbes / kVariants;             // 511
constexpr int kLongSegSlots = kLongSegPositions * kVariants;          // 4,088
constexpr int kLongMaxLen = 4095;                                     // the longest query (the alignment calls')
constexpr int kLongLdsEntries = 2048;                                 // a query's hit entries that fold in LDS
constexpr int kLongLdsSlots = 2 * kLongLdsEntries;                    // ... in a table of twice as many slots

// S(m): the segments of a query of m sorted values (m < 4: none)
constexpr int32_t long_segments(int32_t m) { return m < 4 ? 0 : (m - 3 + kLongSegPositions - 1) / kLongSegPositions; }
// the probe lists per query of a call whose queries have up to max_query_len values: at least one
constexpr int32_t long_lists(int32_t max_query_len) {
    const int32_t s = long_segments(max_query_len > kLongMaxLen ? kLongMaxLen : max_query_len);
    return s < 1 ? 1 : s;
}
// the probe slots of segment s of a query of m values (m < 0: refused, it has none)
constexpr int32_t long_list_slots(int32_t m, int32_t s) {
    if (m < 4 || s < 0) return 0;
    const int32_t left = (m - 3) - s * kLongSegPositions;
    return left <= 0 ? 0 : kVariants * (left < kLongSegPositions ? left : kLongSegPositions);
}
// position i of a query -> its list among the query's, and its first slot in that list
constexpr int32_t long_list_of(int32_t i) { return i / kLongSegPositions; }
constexpr int32_t long_place_of(int32_t i) { return kVariants * (i % kLongSegPositions); }

// The fold's table: open addressing over the next power of two at or above 2 n slots (n: the entries to fold; at least
// 2 slots), keyed by id + 1, the home slot the top bits of a multiplicative hash.
constexpr uint32_t long_table_slots(int64_t n) {
    uint32_t s = 2;
    while ((int64_t)s < 2 * n) s <<= 1;
    return s;
}
constexpr uint32_t long_table_home(uint32_t key, uint32_t slots) {   // slots: a power of two >= 2
    return (key * 0x9E3779B1u) >> (32 - __builtin_ctz(slots));
}
// the table slots a query gets in the workspace: none where every query folds in LDS (lists x cap <= kLongLdsEntries)
constexpr size_t long_ws_table_slots(int32_t lists_per_query, int32_t cap) {
    const int64_t n = (int64_t)lists_per_query * cap;
    return n <= kLongLdsEntries ? 0 : (size_t)long_table_slots(n);
}

// The regions: those of ws_regions for Q x S lists with the lists' exclusion ids - but 8 probe slots per value, not
// 8 S: the segments partition a query's positions - and behind them the Q tables of 8-byte slots (id + 1, count).
struct WsLongRegions : WsRegions {
    size_t table;
};
inline WsLongRegions ws_long_regions(int32_t Q, int32_t S, int32_t cap, size_t match_bytes, int64_t room) {
    WsLongRegions r;
    static_cast<WsRegions &>(r) = ws_regions(Q, S, true, cap, match_bytes, 0);
    size_t p = r.sv;                                                  // (room 0: the fixed regions end here)
    r.sv = p;      p += al256((size_t)room * sizeof(double));
    r.sp = p;      p += al256((size_t)room * sizeof(int32_t));
    r.probes = p;  p += al256((size_t)room * kVariants * sizeof(double));
    r.table = p;   p += al256((size_t)Q * long_ws_table_slots(S, cap) * 2 * sizeof(int32_t));
    r.end = p;
    return r;
}
inline size_t ws_long_bytes(int32_t Q, int32_t S, int32_t cap, size_t match_bytes, int64_t keys) {
    return ws_long_regions(Q, S, cap, match_bytes, 0).end + kWsSlack + (size_t)keys * per_key(1);
}
inline int64_t ws_long_room(int32_t Q, int32_t S, int32_t cap, size_t match_bytes, size_t bytes) {
    const size_t fixed = ws_long_bytes(Q, S, cap, match_bytes, 0);
    return bytes < fixed ? -1 : (int64_t)((bytes - fixed) / per_key(1));
}

// ---- the workspace of tvz_align_candidates_sharded ----
// In front, behind a base aligned up to 256: the rank's own block int32[Q][C + 1][2] and the gathered ones
// int32[max(n_ranks, 1)][Q][C + 1][2]; behind them, from `plain` on (a multiple of 256 from the aligned base, so that
// its own alignment costs nothing), the whole workspace of the plain call.  `cols` = 3: the same front with the rows of
// tvz_align_candidates_rates_sharded (include/tvz_gap_rates_shards.h), the rates call's workspace behind it.
struct ShardWsRegions {              // byte offsets from the aligned base
    size_t local, gathered, plain;
};
inline size_t block_bytes(int32_t Q, int32_t C, int cols = 2) { return (size_t)Q * ((size_t)C + 1) * (size_t)cols * sizeof(int32_t); }
inline ShardWsRegions ws_shard_regions(int32_t Q, int32_t C, int32_t n_ranks, int cols = 2) {
    ShardWsRegions r;
    const size_t n = (size_t)(n_ranks > 1 ? n_ranks : 1);
    size_t p = 0;
    r.local = p;     p += al256(block_bytes(Q, C, cols));
    r.gathered = p;  p += al256(n * block_bytes(Q, C, cols));
    r.plain = p;
    return r;
}
// what the front costs a caller's buffer at most: its regions and the base's alignment
inline size_t ws_shard_front_bytes(int32_t Q, int32_t C, int32_t n_ranks, int cols = 2) {
    return ws_shard_regions(Q, C, n_ranks, cols).plain + 255;
}
// A buffer of `bytes` at address `base` -> where the front starts, and the plain call's part behind it.  That part is
// given bytes - ws_shard_front_bytes (0 if the front does not fit) whatever the base's alignment cost, so that a
// buffer is refused one byte below the sizing function's answer at every base; it ends inside the buffer.
struct ShardWs {
    uintptr_t front, plain;
    size_t plain_bytes;
};
inline ShardWs ws_shard_carve(uintptr_t base, size_t bytes, int32_t Q, int32_t C, int32_t n_ranks, int cols = 2) {
    ShardWs s;
    const size_t front = ws_shard_front_bytes(Q, C, n_ranks, cols);
    s.front = (uintptr_t)al256((size_t)base);
    s.plain = s.front + ws_shard_regions(Q, C, n_ranks, cols).plain;
    s.plain_bytes = bytes > front ? bytes - front : 0;
    return s;
}

}  // namespace tvz_gap
