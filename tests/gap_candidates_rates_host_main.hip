// Stand-alone host program (its own main) for tests/test_gap_candidates_rates_cpu.py: the host code of
// tvz_align_candidates_rates, built for the HOST only with -fsanitize=address,undefined and run without a GPU.  It
// includes the library's translation unit, so the functions under test are the product's own, not copies.
//   - the workspace of the call carved over a real host buffer of the sizing export's byte count at bases misaligned by
//     0, 8 and 248 bytes, for n_rates 1 and 8: every region lies inside the buffer, in order, none overlapping, and is
//     written to its end; the room the call finds in that buffer is the key count it was sized for;
//   - the sizing export's refusals, and the refusals of the call that return before any HIP call, in their order.
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

void carve(int32_t Q, int32_t max_len, int64_t keys, int32_t R, int32_t cap, int32_t C, size_t misalign) {
    const size_t need = tvz_align_candidates_rates_workspace_bytes(Q, max_len, keys, R, cap, C);
    CHECK(need > 0);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *given = buf.data() + misalign;
    const size_t lists = (size_t)Q * R;
    const size_t match_bytes = candidates_match_bytes((int32_t)lists, max_len);
    const int64_t want = std::max<int64_t>(keys > 0 ? keys : (int64_t)Q * max_len, max_len);
    const int64_t room = tvz_gap::ws_room(Q, R, true, cap, match_bytes, need);
    CHECK(room == want);
    CHECK(tvz_gap::ws_room(Q, R, true, cap, match_bytes, need - 1) == want - 1 || want == 0);
    const tvz_gap::WsRegions r = tvz_gap::ws_regions(Q, R, true, cap, match_bytes, room);
    unsigned char *base = reinterpret_cast<unsigned char *>(al256(reinterpret_cast<uintptr_t>(given)));
    const size_t at[] = {r.hits, r.hits_n, r.p_off, r.excl, r.match, r.qm, r.sv, r.sp, r.probes, r.end};
    const size_t bytes[] = {lists * cap * 12, lists * 4, (lists + 1) * 8, lists * 4, match_bytes, (size_t)Q * 4,
                            (size_t)room * 8, (size_t)room * 4, (size_t)room * 64 * R};
    for (int i = 0; i < 9; ++i) {
        CHECK(at[i] % 256 == 0 && at[i] + bytes[i] <= at[i + 1]);
        CHECK(base + at[i] >= given && base + at[i] + bytes[i] <= given + need);
        if (base + at[i] + bytes[i] <= given + need) memset(base + at[i], 0x5a + i, bytes[i]);   // (ASan: inside the vector)
    }
    CHECK(base + r.end <= given + need);
    // the lookup's own part is what its sizing function asks for Q R probe lists of the longest length
    CHECK(match_bytes == tvz_match_workspace_bytes((int32_t)lists, tvz_gap::max_probe_len(max_len), 0, 0, 1));
    // at one rate the call asks for the plain call's bytes and the expanded exclusions
    if (R == 1) {
        const size_t plain = tvz_align_candidates_workspace_bytes(Q, max_len, keys, cap, C);
        CHECK(need == plain + al256((size_t)Q * 4));
    }
}

}  // namespace

int main() {
    for (size_t misalign : {(size_t)0, (size_t)8, (size_t)248}) {
        for (int32_t R : {1, 8}) {
            carve(1, 200, 0, R, 4096, 16, misalign);
            carve(16, 4095, 0, R, 64, 64, misalign);
            carve(70, 40, 1234, R, 17, 1, misalign);
            carve(1, 0, 0, R, 1, 1, misalign);
            carve(3, 514, 515, R, 300, 64, misalign);
            carve(65535 / R, 4, 70000, R, 1, 1, misalign);
        }
    }
    CHECK(tvz_align_candidates_rates_workspace_bytes(0, 10, 0, 3, 16, 16) > 0);
    CHECK(tvz_align_candidates_rates_workspace_bytes(2, 10, 0, 3, 16, 16) > tvz_align_candidates_rates_workspace_bytes(2, 10, 0, 2, 16, 16));
    CHECK(tvz_align_candidates_rates_workspace_bytes(2, 10, 21, 3, 16, 16) > tvz_align_candidates_rates_workspace_bytes(2, 10, 20, 3, 16, 16));
    CHECK(tvz_align_candidates_rates_workspace_bytes(21845, 4, 0, 3, 1, 1) > 0);          // 65,535 probe lists
    const int32_t bad[][6] = {{-1, 10, 0, 1, 16, 16}, {1, -1, 0, 1, 16, 16}, {1, 10, -1, 1, 16, 16}, {1, 10, 0, 1, 16, 0},
                              {1, 10, 0, 1, 16, 65}, {1, 10, 0, 1, 15, 16}, {1, 4096, 0, 1, 16, 16}, {65536, 10, 0, 1, 16, 16},
                              {1, 10, 0, 0, 16, 16}, {1, 10, 0, 9, 16, 16}, {1, 10, 0, -1, 16, 16}, {8192, 10, 0, 8, 16, 16},
                              {21846, 4, 0, 3, 1, 1}};
    for (const auto &b : bad) CHECK(tvz_align_candidates_rates_workspace_bytes(b[0], b[1], b[2], b[3], b[4], b[5]) == 0);
    // ---- what the call refuses before any HIP call, one step of the order at a time (NULL handle: the last of them)
    const double ok[8] = {1.0, 0.96, 1.25, 1.0, 1.0, 1.0, 1.0, 1.0};
    const double nan_rate[2] = {1.0, std::nan("")}, zero_rate[1] = {0.0}, inf_rate[1] = {HUGE_VAL}, neg_rate[1] = {-1.0};
    auto call = [&](int32_t Q, int32_t L, const double *rates, int32_t R, int32_t min_count, int32_t cap, int32_t C) {
        return tvz_align_candidates_rates(nullptr, nullptr, nullptr, Q, L, rates, R, min_count, nullptr, cap, C, nullptr, nullptr, 0,
                                          nullptr);
    };
    CHECK(call(1, 4, nullptr, 0, 0, 1, 0) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "C=0"));
    CHECK(call(1, 4, nullptr, 0, 0, 15, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "cap=15"));
    CHECK(call(1, 4, nullptr, 0, 0, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "min_count 0"));
    CHECK(call(1, 4096, nullptr, 0, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "max_query_len 4096"));
    CHECK(call(70000, 4, nullptr, 0, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "n_rates=0"));
    CHECK(call(70000, 4, ok, 9, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "n_rates=9"));
    CHECK(call(70000, 4, nullptr, 2, 2, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "h_rates is NULL"));
    CHECK(call(70000, 4, nan_rate, 2, 2, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "rate 1 is"));
    CHECK(call(1, 4, zero_rate, 1, 2, 16, 16) == TVZ_ERR_INVALID && call(1, 4, inf_rate, 1, 2, 16, 16) == TVZ_ERR_INVALID &&
          call(1, 4, neg_rate, 1, 2, 16, 16) == TVZ_ERR_INVALID);
    CHECK(call(8192, 4, ok, 8, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "probe lists"));
    CHECK(call(21846, 4, ok, 3, 2, 16, 16) == TVZ_ERR_UNSUPPORTED && std::strstr(tvz_last_error(), "probe lists"));
    CHECK(call(21845, 4, ok, 3, 2, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "corpus is NULL"));
    CHECK(call(1, 4, ok, 8, 2, 16, 16) == TVZ_ERR_INVALID && std::strstr(tvz_last_error(), "corpus is NULL"));
    if (g_bad) return 1;
    std::printf("HOST_OK\n");
    return 0;
}
