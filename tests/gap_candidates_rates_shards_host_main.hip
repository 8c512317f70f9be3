// Stand-alone host program (its own main) for tests/test_gap_candidates_rates_shards_cpu.py: the host code of the rates
// candidates call over a sharded table, built for the HOST only with -fsanitize=address,undefined and run without a GPU.
// It includes the library's translation unit, so the functions under test are the product's own, not copies.
//   - the workspace of tvz_align_candidates_rates_sharded carved (tvz_gap::ws_shard_carve with 3 columns, tvz_gap_codes.h) over a
//     real host buffer of the sizing export's byte count at bases misaligned by 0, 8 and 248 bytes, for 1 and 8 rates
//     and 1 and 16 ranks: the rank's own block, the gathered blocks and every region of the rates call behind them lie
//     inside the buffer, in order, none overlapping, and are written to their ends; one byte less and the rates call's
//     part is one byte short;
//   - the sizing export's formula and zeros;
//   - the refusals of the merge and of the shards call that return before any HIP call, and their order.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../tvidz_amd/csrc/tvz_match.hip"

namespace {

int g_bad = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++g_bad;                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
        }                                                                  \
    } while (0)

void carve(int32_t Q, int32_t max_len, int64_t keys, int32_t R, int32_t cap, int32_t C, int32_t n_ranks, size_t misalign) {
    const size_t rates = tvz_align_candidates_rates_workspace_bytes(Q, max_len, keys, R, cap, C);
    const size_t need = tvz_align_candidates_rates_sharded_workspace_bytes(Q, max_len, keys, R, cap, C, n_ranks);
    const size_t n = (size_t)std::max(n_ranks, 1), block = (size_t)Q * ((size_t)C + 1) * 12;
    CHECK(rates > 0 && need == rates + tvz_gap::al256(block) + tvz_gap::al256(n * block) + 255);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *given = buf.data() + misalign, *end = given + need;
    const tvz_gap::ShardWs s = tvz_gap::ws_shard_carve(reinterpret_cast<uintptr_t>(given), need, Q, C, n_ranks, 3);
    const tvz_gap::ShardWsRegions r = tvz_gap::ws_shard_regions(Q, C, n_ranks, 3);
    unsigned char *front = reinterpret_cast<unsigned char *>(s.front), *pl = reinterpret_cast<unsigned char *>(s.plain);
    CHECK(s.front % 256 == 0 && s.plain % 256 == 0 && front >= given && front < given + 256);
    CHECK(r.local == 0 && r.local + block <= r.gathered && r.gathered + n * block <= r.plain && pl == front + r.plain);
    CHECK(s.plain_bytes == rates && pl + s.plain_bytes <= end);
    if (pl + s.plain_bytes <= end) {                                      // (ASan: every write inside the vector)
        memset(front + r.local, 0x11, block);
        memset(front + r.gathered, 0x22, n * block);
    }
    // the rates call's part, laid out from s.plain on as tvz_align_candidates_rates lays a caller's buffer out
    const size_t lists = (size_t)Q * R;
    const size_t match_bytes = candidates_match_bytes((int32_t)lists, max_len);
    const int64_t want = std::max<int64_t>(keys > 0 ? keys : (int64_t)Q * max_len, max_len);
    const int64_t room = tvz_gap::ws_room(Q, R, true, cap, match_bytes, s.plain_bytes);
    CHECK(room == want);
    const tvz_gap::WsRegions w = tvz_gap::ws_regions(Q, R, true, cap, match_bytes, room);
    unsigned char *base = reinterpret_cast<unsigned char *>(al256(s.plain));
    CHECK(base == pl);                                                    // (its own alignment costs nothing)
    const size_t at[] = {w.hits, w.hits_n, w.p_off, w.excl, w.match, w.qm, w.sv, w.sp, w.probes, w.end};
    const size_t bytes[] = {lists * cap * 12, lists * 4, (lists + 1) * 8, lists * 4, match_bytes, (size_t)Q * 4,
                            (size_t)room * 8, (size_t)room * 4, (size_t)room * 64 * R};
    for (int i = 0; i < 9; ++i) {
        CHECK(at[i] + bytes[i] <= at[i + 1] && base + at[i] + bytes[i] <= end);
        if (base + at[i] + bytes[i] <= end) memset(base + at[i], 0x5a + i, bytes[i]);
    }
    CHECK(base + w.end <= end);
    // the front is still what it was: the rates call's part never reaches back into it
    CHECK(block == 0 || (front[r.local] == 0x11 && front[r.gathered + n * block - 1] == 0x22));
    // one byte less: the rates call's part is one byte short of what it needs, and the room one key short
    const tvz_gap::ShardWs less = tvz_gap::ws_shard_carve(reinterpret_cast<uintptr_t>(given), need - 1, Q, C, n_ranks, 3);
    CHECK(less.plain_bytes == rates - 1);
    CHECK(tvz_gap::ws_room(Q, R, true, cap, match_bytes, less.plain_bytes) == want - 1 || want == 0);
    CHECK(tvz_gap::ws_shard_carve(reinterpret_cast<uintptr_t>(given), 17, Q, C, n_ranks, 3).plain_bytes == 0);
}

}  // namespace

int main() {
    for (size_t misalign : {(size_t)0, (size_t)8, (size_t)248}) {
        for (int32_t R : {1, 8}) {
            for (int32_t n_ranks : {1, 16}) {
                carve(1, 200, 0, R, 4096, 16, n_ranks, misalign);
                carve(16, 4095, 0, R, 64, 64, n_ranks, misalign);
                carve(70, 40, 1234, R, 17, 1, n_ranks, misalign);
                carve(1, 0, 0, R, 1, 1, n_ranks, misalign);
                carve(3, 514, 515, R, 300, 64, n_ranks, misalign);
            }
        }
    }
    // ---- the sizing export: 0 where the rates one answers 0, and for n_ranks < 0; n_ranks 0 is sized as one rank
    auto size = tvz_align_candidates_rates_sharded_workspace_bytes;
    CHECK(size(2, 10, 0, 3, 16, 16, -1) == 0);
    CHECK(size(2, 10, 0, 3, 16, 16, 0) == size(2, 10, 0, 3, 16, 16, 1));
    CHECK(size(2, 10, 0, 3, 16, 16, 2) > size(2, 10, 0, 3, 16, 16, 1));
    const int32_t bad[][6] = {{-1, 10, 0, 1, 16, 16}, {1, -1, 0, 1, 16, 16}, {1, 10, -1, 1, 16, 16}, {1, 10, 0, 1, 16, 0},
                              {1, 10, 0, 1, 16, 65}, {1, 10, 0, 1, 15, 16}, {1, 4096, 0, 1, 16, 16}, {65536, 10, 0, 1, 16, 16},
                              {1, 10, 0, 0, 16, 16}, {1, 10, 0, 9, 16, 16}, {8192, 10, 0, 8, 16, 16}, {21846, 4, 0, 3, 1, 1}};
    for (const auto &b : bad) CHECK(size(b[0], b[1], b[2], b[3], b[4], b[5], 4) == 0);
    // ---- what the merge and the shards call refuse before any HIP call
    int32_t *g = reinterpret_cast<int32_t *>(0x10000), *o = reinterpret_cast<int32_t *>(0x80000);
    auto merge = tvz_align_candidates_rates_merge;
    CHECK(merge(g, 0, 1, 16, o, nullptr) == TVZ_ERR_UNSUPPORTED && merge(g, 17, 1, 16, o, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(merge(g, 1, 1, 0, o, nullptr) == TVZ_ERR_UNSUPPORTED && merge(g, 1, 1, 65, o, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(merge(g, 0, -1, 16, nullptr, nullptr) == TVZ_ERR_UNSUPPORTED);                    // (the list count stands first)
    CHECK(merge(g, 1, -1, 16, o, nullptr) == TVZ_ERR_INVALID);
    CHECK(merge(nullptr, 1, 1, 16, o, nullptr) == TVZ_ERR_INVALID && merge(g, 1, 1, 16, nullptr, nullptr) == TVZ_ERR_INVALID);
    const int32_t *g_odd = reinterpret_cast<const int32_t *>(0x10002);
    CHECK(merge(g_odd, 1, 1, 16, o, nullptr) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "4-byte aligned"));
    CHECK(merge(g, 1, 1, 16, reinterpret_cast<int32_t *>(0x80001), nullptr) == TVZ_ERR_INVALID);
    CHECK(merge(g, 2, 3, 16, g + 2 * 3 * 17 * 3 - 3, nullptr) == TVZ_ERR_INVALID);         // its last row inside
    CHECK(merge(g, 2, 3, 16, g, nullptr) == TVZ_ERR_INVALID);
    CHECK(merge(nullptr, 1, 0, 16, nullptr, nullptr) == TVZ_OK);
    const double ok[3] = {1.0, 0.96, 1.25};
    tvz_corpus *none[2] = {nullptr, nullptr};
    auto shards = [&](tvz_corpus *const *hs, int32_t n, int32_t Q, const double *rates, int32_t R, int32_t min_count, int32_t cap,
                      int32_t C) {
        return tvz_align_candidates_rates_shards(hs, n, nullptr, nullptr, Q, 4, rates, R, min_count, nullptr, cap, C, g, o, nullptr, 0,
                                                 nullptr);
    };
    CHECK(shards(nullptr, 17, 70000, nullptr, 0, 0, 1, 0) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "C=0"));
    CHECK(shards(nullptr, 17, 70000, nullptr, 0, 0, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "min_count 0"));
    CHECK(shards(nullptr, 17, 70000, nullptr, 0, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "n_rates=0"));
    CHECK(shards(nullptr, 17, 70000, nullptr, 3, 2, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "h_rates is NULL"));
    CHECK(shards(nullptr, 17, 70000, ok, 3, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "probe lists"));
    CHECK(shards(nullptr, 17, 1, ok, 3, 2, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "no shards"));
    CHECK(shards(none, 17, 1, ok, 3, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "17 lists"));
    CHECK(shards(none, 2, 1, ok, 3, 2, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "shard 0 is NULL"));
    if (g_bad) return 1;
    std::printf("HOST_OK\n");
    return 0;
}
