// Stand-alone host program (its own main) for tests/test_gap_candidates_long_cpu.py: the host arithmetic of
// tvz_align_candidates_long, built for the HOST with -fsanitize=address,undefined and run without a GPU.  It includes
// tvz_gap_codes.h alone - the header the library's kernels and its host code share.
//   - the segment arithmetic over every m in 0..4,096: S(m), the lists' slots, every position's list and place;
//   - the fold's table: its size and the home slots;
//   - the workspace carved over a real host buffer at bases misaligned by 0, 8 and 248 bytes: every region lies inside
//     the buffer, in order, none overlapping, and is written to its end.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../tvidz_amd/csrc/tvz_gap_codes.h"

namespace {

int g_bad = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++g_bad;                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
        }                                                                  \
    } while (0)

using namespace tvz_gap;

void segments() {
    static_assert(kLongSegPositions == 511 && kLongSegSlots == 4088 && kLongSegSlots <= kMaxProbes, "a segment fits the lookup");
    static_assert(long_segments(3) == 0 && long_segments(4) == 1 && long_segments(514) == 1 && long_segments(515) == 2 &&
                      long_segments(1025) == 2 && long_segments(1026) == 3 && long_segments(4095) == 9,
                  "S(m)");
    static_assert(kLongLdsSlots >= 2 * kLongLdsEntries, "the LDS table has twice the entries' slots");
    for (int32_t m = -1; m <= 4096; ++m) {
        const int32_t S = long_segments(m), positions = m < 4 ? 0 : m - 3;
        CHECK(S == (positions + 510) / 511);
        CHECK(long_lists(m) == (m > 4095 ? 9 : (S < 1 ? 1 : S)) && long_lists(m) <= 9);
        int64_t sum = 0;
        for (int32_t s = 0; s < 12; ++s) {
            const int32_t slots = long_list_slots(m, s);
            CHECK(slots >= 0 && slots <= kLongSegSlots && slots % kVariants == 0);
            CHECK((slots > 0) == (s < S));
            if (s + 1 < S) CHECK(slots == kLongSegSlots);
            sum += slots;
        }
        CHECK(sum == (int64_t)kVariants * positions);
        std::vector<unsigned char> seen((size_t)sum, 0);             // every slot of every list is some position's, once
        for (int32_t i = 0; i < positions; ++i) {
            const int32_t l = long_list_of(i), at = long_place_of(i);
            CHECK(l >= 0 && l < S && at >= 0 && at + kVariants <= long_list_slots(m, l));
            size_t before = 0;
            for (int32_t s = 0; s < l; ++s) before += (size_t)long_list_slots(m, s);
            for (int v = 0; v < kVariants; ++v) {
                CHECK(before + at + v < seen.size() && !seen[before + at + v]);
                if (before + at + v < seen.size()) seen[before + at + v] = 1;
            }
        }
        for (unsigned char x : seen) CHECK(x == 1);
    }
    CHECK(long_list_slots(-5, 0) == 0 && long_list_slots(515, -1) == 0);
}

void table() {
    CHECK(long_table_slots(0) == 2 && long_table_slots(1) == 2 && long_table_slots(2) == 4 && long_table_slots(3) == 8);
    CHECK(long_table_slots(2047) == 4096 && long_table_slots(2048) == 4096 && long_table_slots(2049) == 8192);
    CHECK(long_table_slots(9 * 4096) == 131072 && long_table_slots(525000) == (1u << 21));
    for (uint32_t slots = 2; slots <= (1u << 21); slots <<= 1)
        for (uint32_t key : {1u, 2u, 3u, 4097u, 0x7fffffffu, 0x80000000u}) CHECK(long_table_home(key, slots) < slots);
    CHECK(long_ws_table_slots(1, 2048) == 0 && long_ws_table_slots(1, 2049) == 8192 && long_ws_table_slots(9, 4096) == 131072 &&
          long_ws_table_slots(2, 1024) == 0);
}

void carve(int32_t Q, int32_t max_len, int64_t keys, int32_t cap, size_t match_bytes, size_t misalign) {
    const int32_t S = long_lists(max_len);
    const size_t need = ws_long_bytes(Q, S, cap, match_bytes, keys);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *given = buf.data() + misalign;
    const size_t lists = (size_t)Q * S;
    const int64_t room = ws_long_room(Q, S, cap, match_bytes, need);
    CHECK(room == keys);
    CHECK(keys == 0 || ws_long_room(Q, S, cap, match_bytes, need - 1) == keys - 1);
    CHECK(ws_long_room(Q, S, cap, match_bytes, ws_long_bytes(Q, S, cap, match_bytes, 0) - 1) == -1);
    const WsLongRegions r = ws_long_regions(Q, S, cap, match_bytes, room);
    unsigned char *base = reinterpret_cast<unsigned char *>(al256(reinterpret_cast<uintptr_t>(given)));
    const size_t at[] = {r.hits, r.hits_n, r.p_off, r.excl, r.match, r.qm, r.sv, r.sp, r.probes, r.table, r.end};
    const size_t bytes[] = {lists * cap * 12, lists * 4, (lists + 1) * 8, lists * 4, match_bytes, (size_t)Q * 4,
                            (size_t)room * 8, (size_t)room * 4, (size_t)room * 64, (size_t)Q * long_ws_table_slots(S, cap) * 8};
    for (int i = 0; i < 10; ++i) {
        CHECK(at[i] % 256 == 0 && at[i] + bytes[i] <= at[i + 1]);
        CHECK(base + at[i] >= given && base + at[i] + bytes[i] <= given + need);
        if (base + at[i] + bytes[i] <= given + need) memset(base + at[i], 0x5a + i, bytes[i]);   // (ASan: inside the vector)
    }
    CHECK(base + r.end <= given + need);
    // the probes hold every list of every query the room admits: 8 slots per value, whatever S
    CHECK((size_t)room * 64 >= (size_t)kVariants * 8 * (size_t)(room > 3 ? room - 3 : 0));
}

}  // namespace

int main() {
    segments();
    table();
    for (size_t misalign : {(size_t)0, (size_t)8, (size_t)248}) {
        carve(1, 200, 200, 4096, 1000, misalign);
        carve(1, 4095, 4095, 4096, 123457, misalign);
        carve(16, 1500, 16 * 1500, 64, 77, misalign);
        carve(3, 515, 1030, 1025, 0, misalign);
        carve(7, 1026, 1026, 17, 4096, misalign);
        carve(70, 40, 1234, 17, 99, misalign);
        carve(1, 0, 0, 1, 1, misalign);
    }
    if (g_bad) return 1;
    std::printf("HOST_OK\n");
    return 0;
}
