// Stand-alone host program (its own main) for tests/test_align_parts_cpu.py: the sizing and carving code of
// tvz_align_parts, built for the HOST only with -fsanitize=address,undefined and run without a GPU.  It includes the
// library's translation unit, so the functions under test are the product's own, not copies.
//   - walks align_parts_ws_layout + tol_ws_layout over a real host buffer at bases misaligned by 0, 8 and 248 bytes:
//     every region lies inside the buffer of the sizing export's byte count, in order, none overlapping, and is
//     written to its end - so the sizing export equals the walk;
//   - the sizing export's refusals and its growth with every argument;
//   - the refusals of the call that return before any HIP call.
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

struct Region {
    unsigned char *p;
    size_t bytes;
};

void carve(int32_t Q, int32_t max_len, int64_t keys, int32_t k, int32_t max_parts, size_t misalign) {
    const size_t need = tvz_align_parts_workspace_bytes(Q, max_len, keys, k, max_parts);
    CHECK(need > 0);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *base = buf.data() + misalign;
    Carver cv(base);
    const AlignPartsWs w = align_parts_ws_layout(cv, Q, k, max_parts);
    {   // the sizing export is the same walk from NULL, + the sorted queries' part
        Carver from_null(nullptr);
        align_parts_ws_layout(from_null, Q, k, max_parts);
        CHECK(need == from_null.fixed() + tol_ws_bytes(Q, std::max<int64_t>(keys > 0 ? keys : (int64_t)Q * max_len, max_len)));
    }
    const int64_t room = tol_ws_room(Q, need - cv.fixed());
    CHECK(room >= std::max<int64_t>(keys, max_len));
    const size_t pairs = (size_t)Q * (size_t)k;
    std::vector<Region> r = {{(unsigned char *)w.counts, pairs * 4},
                             {(unsigned char *)w.slots, pairs * TVZ_ALIGN_PARTS_MAX_ROWS * 8},
                             {(unsigned char *)w.scratch, pairs * TVZ_ALIGN_PARTS_MAX_ROWS * (size_t)(1 + max_parts) * 6 * 4}};
    const TolWs t = tol_ws_layout(cv, Q, room);
    r.push_back({(unsigned char *)t.qm, (size_t)Q * 4});
    r.push_back({(unsigned char *)t.sv, (size_t)room * 8});
    r.push_back({(unsigned char *)t.sp, (size_t)room * 4});
    unsigned char *at = base;
    for (const Region &x : r) {
        CHECK(x.p >= at && ((uintptr_t)x.p & 255) == 0 && x.p + x.bytes <= base + need);
        if (x.p >= at && x.p + x.bytes <= base + need) memset(x.p, 0x5a, x.bytes);     // (ASan watches the vector's end)
        at = x.p + x.bytes;
    }
}

}  // namespace

int main() {
    for (size_t mis : {(size_t)0, (size_t)8, (size_t)248})
        for (int32_t Q : {1, 3, 64})
            for (int32_t k : {1, 5, 64})
                for (int32_t max_parts = 1; max_parts <= TVZ_ALIGN_MAX_PARTS; ++max_parts) {
                    carve(Q, 40, 0, k, max_parts, mis);
                    carve(Q, 4095, (int64_t)Q * 100 + 4095, k, max_parts, mis);
                }
    CHECK(kApMaxParts == TVZ_ALIGN_MAX_PARTS && kApMaxRows == TVZ_ALIGN_PARTS_MAX_ROWS && ap_words(4) == 30);
    // the size: the sorted queries' + the three regions, each rounded to 256 bytes; 0 for what the call refuses; monotone
    for (int32_t Q : {0, 1, 2, 7, 64})
        for (int32_t len : {0, 1, 40, 4095})
            for (int32_t k : {1, 2, 16, 64})
                for (int32_t P : {1, 2, 3, 4}) {
                    const size_t sz = tvz_align_parts_workspace_bytes(Q, len, 0, k, P);
                    const size_t regions = (size_t)Q * k * (4 + 64 + 8 * (size_t)(1 + P) * 24);
                    const size_t sorted = tvz_match_tol_workspace_bytes(Q, len, std::max<int64_t>((int64_t)Q * len, len));
                    CHECK(sz >= sorted + regions && sz <= sorted + regions + 4 * 256);
                    CHECK(tvz_align_parts_workspace_bytes(Q + 1, len, 0, k, P) >= sz);
                    CHECK(tvz_align_parts_workspace_bytes(Q, len + 1, 0, k, P) >= sz);
                    CHECK(tvz_align_parts_workspace_bytes(Q, len, 0, k + 1, P) >= sz);
                    CHECK(P == 4 || tvz_align_parts_workspace_bytes(Q, len, 0, k, P + 1) >= sz);
                    CHECK(tvz_align_parts_workspace_bytes(Q, len, (int64_t)Q * len + 100, k, P) >= sz);
                }
    CHECK(tvz_align_parts_workspace_bytes(-1, 1, 0, 1, 1) == 0 && tvz_align_parts_workspace_bytes(1, -1, 0, 1, 1) == 0);
    CHECK(tvz_align_parts_workspace_bytes(1, 1, -1, 1, 1) == 0 && tvz_align_parts_workspace_bytes(1, 1, 0, 0, 1) == 0);
    CHECK(tvz_align_parts_workspace_bytes(1, 1, 0, 1, 0) == 0 && tvz_align_parts_workspace_bytes(1, 1, 0, 1, 5) == 0);
    // refusals that return before any HIP call: the parameters first, the handle behind them
    const double rates[2] = {1.0, 0.96}, bad_rates[2] = {1.0, -1.0};
    auto call = [&](const double *r, int32_t n, int32_t k, int32_t len, int32_t min_votes, int32_t P, double eps, double mo) {
        return tvz_align_parts(nullptr, nullptr, nullptr, 1, len, nullptr, 1, 1, k, eps, mo, r, n, min_votes, P, nullptr, nullptr, 0,
                               nullptr);
    };
    CHECK(call(rates, 0, 4, 10, 1, 2, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED && call(rates, 9, 4, 10, 1, 2, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED);
    CHECK(call(nullptr, 1, 4, 10, 1, 2, 0.1, 1.0) == TVZ_ERR_INVALID && call(bad_rates, 2, 4, 10, 1, 2, 0.1, 1.0) == TVZ_ERR_INVALID);
    CHECK(call(rates, 2, 4, 10, 0, 2, 0.1, 1.0) == TVZ_ERR_INVALID);
    CHECK(call(rates, 2, 0, 10, 1, 2, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED && call(rates, 2, 65, 10, 1, 2, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED);
    CHECK(call(rates, 2, 4, 4096, 1, 2, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED);
    CHECK(call(rates, 2, 4, 10, 1, 0, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED && call(rates, 2, 4, 10, 1, 5, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED);
    CHECK(call(rates, 2, 4, 10, 1, 2, 0.0, 1.0) == TVZ_ERR_INVALID && call(rates, 2, 4, 10, 1, 2, 0.1, -1.0) == TVZ_ERR_INVALID);
    CHECK(call(rates, 2, 4, 10, 1, 2, 1.0, 4194305.0) == TVZ_ERR_UNSUPPORTED);
    CHECK(call(rates, 2, 4, 10, 1, 2, 1.0, 4194304.0) == TVZ_ERR_INVALID);                 // good parameters: the NULL handle
    std::printf(g_bad ? "FAILED %d\n" : "HOST_OK\n", g_bad);
    return g_bad ? 1 : 0;
}
