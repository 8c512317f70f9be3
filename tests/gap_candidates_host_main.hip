// Stand-alone host program (its own main) for tests/test_gap_candidates_cpu.py: the host code of the gap index, built
// for the HOST only with -fsanitize=address,undefined and run without a GPU.  It includes the library's translation
// unit, so the functions under test are the product's own, not copies.
//   - tvz_gap::row_codes over the rows given on standard input (line 1: gap_eps as a hex float; then per row its count
//     and its keys as the handle keeps them: canonical bit patterns as decimal int64, sorted as integers): the codes are
//     printed, one line per row, for the test to hold against the reference;
//   - the workspace of tvz_align_candidates carved over a real host buffer of the sizing export's byte count at bases
//     misaligned by 0, 8 and 248 bytes: every region lies inside the buffer, in order, none overlapping, and is written
//     to its end; the room the call finds in that buffer is the key count it was sized for;
//   - the sizing export's refusals, and the refusals of the call that return before any HIP call.
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

void carve(int32_t Q, int32_t max_len, int64_t keys, int32_t cap, int32_t C, size_t misalign) {
    const size_t need = tvz_align_candidates_workspace_bytes(Q, max_len, keys, cap, C);
    CHECK(need > 0);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *given = buf.data() + misalign;
    const size_t match_bytes = candidates_match_bytes(Q, max_len);
    const int64_t want = std::max<int64_t>(keys > 0 ? keys : (int64_t)Q * max_len, max_len);
    const int64_t room = tvz_gap::ws_room(Q, 1, false, cap, match_bytes, need);
    CHECK(room == want);
    CHECK(tvz_gap::ws_room(Q, 1, false, cap, match_bytes, need - 1) == want - 1 || want == 0);
    const tvz_gap::WsRegions r = tvz_gap::ws_regions(Q, 1, false, cap, match_bytes, room);
    unsigned char *base = reinterpret_cast<unsigned char *>(al256(reinterpret_cast<uintptr_t>(given)));
    const size_t at[] = {r.hits, r.hits_n, r.p_off, r.match, r.qm, r.sv, r.sp, r.probes, r.end};
    const size_t bytes[] = {(size_t)Q * cap * 12, (size_t)Q * 4, ((size_t)Q + 1) * 8, match_bytes, (size_t)Q * 4,
                            (size_t)room * 8, (size_t)room * 4, (size_t)room * 64};
    for (int i = 0; i < 8; ++i) {
        CHECK(at[i] % 256 == 0 && at[i] + bytes[i] <= at[i + 1]);
        CHECK(base + at[i] >= given && base + at[i] + bytes[i] <= given + need);
        if (base + at[i] + bytes[i] <= given + need) memset(base + at[i], 0x5a + i, bytes[i]);   // (ASan: inside the vector)
    }
    CHECK(base + r.end <= given + need);
    // the lookup's own part is what its sizing function asks for Q probe lists of the longest length
    CHECK(match_bytes == tvz_match_workspace_bytes(Q, tvz_gap::max_probe_len(max_len), 0, 0, 1));
}

}  // namespace

int main() {
    // ---- the codes of the rows on standard input
    double gap_eps = 0.0;
    if (std::scanf("%la", &gap_eps) != 1) return 2;
    std::vector<double> vals, codes;
    long long n;
    while (std::scanf("%lld", &n) == 1) {
        std::vector<int64_t> keys((size_t)n);
        for (long long i = 0; i < n; ++i) {
            long long k;
            if (std::scanf("%lld", &k) != 1) return 2;
            keys[(size_t)i] = k;
        }
        codes.clear();
        const int64_t made = tvz_gap::row_codes(keys.data(), n, gap_eps, vals, codes);
        CHECK(made == (int64_t)codes.size() && made <= std::max<long long>(n - 3, 0));
        std::printf("ROW");
        for (double c : codes) std::printf(" %.0f", c);
        std::printf("\n");
    }
    // ---- the probe slots of a query
    CHECK(tvz_gap::probe_slots(-1) == -1 && tvz_gap::probe_slots(0) == 0 && tvz_gap::probe_slots(3) == 0);
    CHECK(tvz_gap::probe_slots(4) == 8 && tvz_gap::probe_slots(514) == 4088 && tvz_gap::probe_slots(515) == -1);
    CHECK(tvz_gap::max_probe_len(0) == 8 && tvz_gap::max_probe_len(4) == 8 && tvz_gap::max_probe_len(514) == 4088 &&
          tvz_gap::max_probe_len(4095) == 4088);
    // ---- the workspace
    for (size_t misalign : {(size_t)0, (size_t)8, (size_t)248}) {
        carve(1, 200, 0, 4096, 16, misalign);
        carve(16, 4095, 0, 64, 64, misalign);
        carve(70, 40, 1234, 17, 1, misalign);
        carve(1, 0, 0, 1, 1, misalign);
        carve(3, 514, 515, 300, 64, misalign);
        carve(65535, 4, 70000, 1, 1, misalign);
    }
    CHECK(tvz_align_candidates_workspace_bytes(0, 10, 0, 16, 16) > 0);
    CHECK(tvz_align_candidates_workspace_bytes(2, 10, 0, 64, 16) > tvz_align_candidates_workspace_bytes(2, 10, 0, 16, 16));
    CHECK(tvz_align_candidates_workspace_bytes(2, 10, 21, 16, 16) > tvz_align_candidates_workspace_bytes(2, 10, 20, 16, 16));
    const int32_t bad[][5] = {{-1, 10, 0, 16, 16}, {1, -1, 0, 16, 16}, {1, 10, -1, 16, 16}, {1, 10, 0, 16, 0}, {1, 10, 0, 16, 65},
                              {1, 10, 0, 15, 16}, {1, 4096, 0, 16, 16}, {65536, 10, 0, 16, 16}};
    for (const auto &b : bad) CHECK(tvz_align_candidates_workspace_bytes(b[0], b[1], b[2], b[3], b[4]) == 0);
    // ---- what the call and the handle's switch refuse before any HIP call
    CHECK(tvz_align_candidates(nullptr, nullptr, nullptr, 1, 4, 2, nullptr, 16, 0, nullptr, nullptr, 0, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_candidates(nullptr, nullptr, nullptr, 1, 4, 0, nullptr, 16, 16, nullptr, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_candidates(nullptr, nullptr, nullptr, 1, 4, 2, nullptr, 16, 16, nullptr, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_corpus_gap_index(nullptr, 0.1) == TVZ_ERR_INVALID);
    CHECK(tvz_corpus_gap_index_stats(nullptr, nullptr, nullptr) == TVZ_ERR_INVALID);
    if (g_bad) return 1;
    std::printf("HOST_OK\n");
    return 0;
}
