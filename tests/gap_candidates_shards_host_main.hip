// Stand-alone host program (its own main) for tests/test_gap_candidates_shards_cpu.py: the host code of the candidates
// call over a sharded table, built for the HOST only with -fsanitize=address,undefined and run without a GPU.  It
// includes the library's translation unit, so the functions under test are the product's own, not copies.
//   - the workspace of tvz_align_candidates_sharded carved (tvz_gap::ws_shard_carve, tvz_gap_codes.h) over a real host
//     buffer of the sizing export's byte count at bases misaligned by 0, 8 and 248 bytes: the rank's own block, the
//     gathered blocks and every region of the plain call behind them lie inside the buffer, in order, none overlapping,
//     and are written to their ends; one byte less and the plain call's part is one byte short;
//   - the sizing export's formula and refusals;
//   - the refusals of the three calls that return before any HIP call, and their order.
#include <cinttypes>
#include <cstdio>
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

void carve(int32_t Q, int32_t max_len, int64_t keys, int32_t cap, int32_t C, int32_t n_ranks, size_t misalign) {
    const size_t plain = tvz_align_candidates_workspace_bytes(Q, max_len, keys, cap, C);
    const size_t need = tvz_align_candidates_sharded_workspace_bytes(Q, max_len, keys, cap, C, n_ranks);
    const size_t n = (size_t)std::max(n_ranks, 1), block = (size_t)Q * ((size_t)C + 1) * 8;
    CHECK(plain > 0 && need == plain + tvz_gap::al256(block) + tvz_gap::al256(n * block) + 255);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *given = buf.data() + misalign, *end = given + need;
    const tvz_gap::ShardWs s = tvz_gap::ws_shard_carve(reinterpret_cast<uintptr_t>(given), need, Q, C, n_ranks);
    const tvz_gap::ShardWsRegions r = tvz_gap::ws_shard_regions(Q, C, n_ranks);
    unsigned char *front = reinterpret_cast<unsigned char *>(s.front), *pl = reinterpret_cast<unsigned char *>(s.plain);
    CHECK(s.front % 256 == 0 && s.plain % 256 == 0 && front >= given && front < given + 256);
    CHECK(r.local == 0 && r.local + block <= r.gathered && r.gathered + n * block <= r.plain && pl == front + r.plain);
    CHECK(s.plain_bytes == plain && pl + s.plain_bytes <= end);
    if (pl + s.plain_bytes <= end) {                                      // (ASan: every write inside the vector)
        memset(front + r.local, 0x11, block);
        memset(front + r.gathered, 0x22, n * block);
    }
    // the plain call's part, laid out from s.plain on as tvz_align_candidates lays a caller's buffer out
    const size_t match_bytes = candidates_match_bytes(Q, max_len);
    const int64_t want = std::max<int64_t>(keys > 0 ? keys : (int64_t)Q * max_len, max_len);
    const int64_t room = tvz_gap::ws_room(Q, 1, false, cap, match_bytes, s.plain_bytes);
    CHECK(room == want);
    const tvz_gap::WsRegions w = tvz_gap::ws_regions(Q, 1, false, cap, match_bytes, room);
    unsigned char *base = reinterpret_cast<unsigned char *>(al256(s.plain));
    CHECK(base == pl);                                                    // (its own alignment costs nothing)
    const size_t at[] = {w.hits, w.hits_n, w.p_off, w.match, w.qm, w.sv, w.sp, w.probes, w.end};
    const size_t bytes[] = {(size_t)Q * cap * 12, (size_t)Q * 4, ((size_t)Q + 1) * 8, match_bytes, (size_t)Q * 4,
                            (size_t)room * 8, (size_t)room * 4, (size_t)room * 64};
    for (int i = 0; i < 8; ++i) {
        CHECK(at[i] + bytes[i] <= at[i + 1] && base + at[i] + bytes[i] <= end);
        if (base + at[i] + bytes[i] <= end) memset(base + at[i], 0x5a + i, bytes[i]);
    }
    CHECK(base + w.end <= end);
    // the front is still what it was: the plain part never reaches back into it
    CHECK(block == 0 || (front[r.local] == 0x11 && front[r.gathered + n * block - 1] == 0x22));
    // one byte less: the plain call's part is one byte short of what it needs
    const tvz_gap::ShardWs less = tvz_gap::ws_shard_carve(reinterpret_cast<uintptr_t>(given), need - 1, Q, C, n_ranks);
    CHECK(less.plain_bytes == plain - 1);
    CHECK(tvz_gap::ws_shard_carve(reinterpret_cast<uintptr_t>(given), 17, Q, C, n_ranks).plain_bytes == 0);
}

}  // namespace

int main() {
    for (size_t misalign : {(size_t)0, (size_t)8, (size_t)248}) {
        carve(1, 200, 0, 4096, 16, 1, misalign);
        carve(16, 4095, 0, 64, 64, 8, misalign);
        carve(70, 40, 1234, 17, 1, 3, misalign);
        carve(1, 0, 0, 1, 1, 0, misalign);
        carve(3, 514, 515, 300, 64, 16, misalign);
        carve(65535, 4, 70000, 1, 1, 2, misalign);
    }
    // ---- the sizing export: 0 where the plain one answers 0, and for n_ranks < 0; n_ranks 0 is sized as one rank
    CHECK(tvz_align_candidates_sharded_workspace_bytes(2, 10, 0, 16, 16, -1) == 0);
    CHECK(tvz_align_candidates_sharded_workspace_bytes(2, 10, 0, 16, 16, 0) == tvz_align_candidates_sharded_workspace_bytes(2, 10, 0, 16, 16, 1));
    CHECK(tvz_align_candidates_sharded_workspace_bytes(2, 10, 0, 16, 16, 2) > tvz_align_candidates_sharded_workspace_bytes(2, 10, 0, 16, 16, 1));
    const int32_t bad[][5] = {{-1, 10, 0, 16, 16}, {1, -1, 0, 16, 16}, {1, 10, -1, 16, 16}, {1, 10, 0, 16, 0}, {1, 10, 0, 16, 65},
                              {1, 10, 0, 15, 16}, {1, 4096, 0, 16, 16}, {65536, 10, 0, 16, 16}};
    for (const auto &b : bad) CHECK(tvz_align_candidates_sharded_workspace_bytes(b[0], b[1], b[2], b[3], b[4], 4) == 0);
    // ---- what the three calls refuse before any HIP call
    int32_t *g = reinterpret_cast<int32_t *>(0x10000), *o = reinterpret_cast<int32_t *>(0x80000);
    CHECK(tvz_align_candidates_merge(g, 0, 1, 16, o, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates_merge(g, 17, 1, 16, o, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates_merge(g, 1, 1, 0, o, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates_merge(g, 1, 1, 65, o, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates_merge(g, 1, -1, 16, o, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_merge(nullptr, 1, 1, 16, o, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_merge(g, 1, 1, 16, nullptr, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_merge(g + 1, 1, 1, 16, o, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_merge(g, 1, 1, 16, o + 1, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_merge(g, 2, 3, 16, g + 2 * 3 * 17 * 2 - 2, nullptr) == TVZ_ERR_INVALID);      // its last row inside
    CHECK(tvz_align_candidates_merge(g, 2, 3, 16, g, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_merge(nullptr, 1, 0, 16, nullptr, nullptr) == TVZ_OK);
    tvz_corpus *none[2] = {nullptr, nullptr};
    CHECK(tvz_align_candidates_shards(none, 2, nullptr, nullptr, 1, 4, 2, nullptr, 16, 0, g, o, nullptr, 0, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates_shards(nullptr, 2, nullptr, nullptr, 1, 4, 2, nullptr, 16, 16, g, o, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_shards(none, 17, nullptr, nullptr, 1, 4, 2, nullptr, 16, 16, g, o, nullptr, 0, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates_shards(none, 2, nullptr, nullptr, 1, 4, 2, nullptr, 16, 16, g, o, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_sharded(nullptr, nullptr, nullptr, nullptr, 1, 4, 2, nullptr, 16, 0, o, nullptr, 0, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates_sharded(nullptr, nullptr, nullptr, nullptr, 1, 4, 0, nullptr, 16, 16, o, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates_sharded(nullptr, nullptr, nullptr, nullptr, 1, 4, 2, nullptr, 16, 16, o, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    if (g_bad) return 1;
    std::printf("HOST_OK\n");
    return 0;
}
