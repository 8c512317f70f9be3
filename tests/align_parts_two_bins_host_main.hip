// Stand-alone host program (its own main) for tests/test_align_parts_two_bins_cpu.py: the host code of
// tvz_align_parts_flags, built for the HOST only with -fsanitize=address,undefined and run without a GPU.  It includes
// the library's translation unit, so the functions under test are the product's own, not copies.
//   - the flags check: 0 and TVZ_ALIGN_TWO_BINS pass, every other bit is refused with the form's name;
//   - the order of the early checks (check_align_parts_early): the flags behind max_parts, in front of eps / max_offset / B,
//     for the call and for its _shards form, which then goes on to its own refusals;
//   - the carving is unchanged: align_parts_ws_layout + tol_ws_layout over a real host buffer of
//     tvz_align_parts_workspace_bytes at bases misaligned by 0, 8 and 248 bytes, every region inside and written to its
//     end - the flags add no region and no byte.
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

bool said(const char *words) { return std::strstr(tvz_last_error(), words) != nullptr; }

void carve(int32_t Q, int32_t max_len, int64_t keys, int32_t k, int32_t max_parts, size_t misalign) {
    const size_t need = tvz_align_parts_workspace_bytes(Q, max_len, keys, k, max_parts);
    CHECK(need > 0);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *base = buf.data() + misalign;
    Carver cv(base);
    const AlignPartsWs w = align_parts_ws_layout(cv, Q, k, max_parts);
    CHECK(w.local == nullptr && w.gathered == nullptr);
    const int64_t room = tol_ws_room(Q, need - cv.fixed());
    CHECK(room >= std::max<int64_t>(keys, max_len));
    const size_t pairs = (size_t)Q * (size_t)k;
    const TolWs t = tol_ws_layout(cv, Q, room);
    unsigned char *p[] = {(unsigned char *)w.counts, (unsigned char *)w.slots, (unsigned char *)w.scratch, (unsigned char *)t.qm,
                          (unsigned char *)t.sv, (unsigned char *)t.sp};
    const size_t bytes[] = {pairs * 4, pairs * kApMaxRows * 8, pairs * kApMaxRows * (size_t)ap_words(max_parts) * 4, (size_t)Q * 4,
                            (size_t)room * 8, (size_t)room * 4};
    unsigned char *at = base;
    for (int i = 0; i < 6; ++i) {
        CHECK(p[i] >= at && ((uintptr_t)p[i] & 255) == 0 && p[i] + bytes[i] <= base + need);
        if (p[i] >= at && p[i] + bytes[i] <= base + need) memset(p[i], 0x5a + i, bytes[i]);     // (ASan watches the vector's end)
        at = p[i] + bytes[i];
    }
}

}  // namespace

int main() {
    // ---- the flags check itself
    CHECK(kAlignPartsForm.flags == TVZ_ALIGN_TWO_BINS && kAlignPartsForm.exclusive == 0u && kAlTwoBins == TVZ_ALIGN_TWO_BINS);
    CHECK(check_align_flags(kAlignPartsForm, 0u, "") == TVZ_OK && check_align_flags(kAlignPartsForm, TVZ_ALIGN_TWO_BINS, "") == TVZ_OK);
    const uint32_t bad[] = {4u, 1u, 8u | 1u, 0x80000008u, 2u, 16u, ~0u};
    for (uint32_t f : bad) {
        CHECK(check_align_flags(kAlignPartsForm, f, "") == TVZ_ERR_INVALID && said("alignment parts: unknown flag bits 0x"));
    }
    // ---- the early checks' order, on NULL handles and pointers: nothing is dereferenced
    const double rates[2] = {1.0, 0.96}, bad_rates[2] = {1.0, -1.0};
    auto call = [&](const double *r, int32_t n, int32_t k, int32_t len, int32_t min_votes, int32_t P, uint32_t flags, double eps,
                    double mo) {
        return tvz_align_parts_flags(nullptr, nullptr, nullptr, 1, len, nullptr, 1, 1, k, eps, mo, r, n, min_votes, P, flags, nullptr,
                                     nullptr, 0, nullptr);
    };
    auto shards = [&](tvz_corpus *const *hs, int32_t n_shards, const double *r, int32_t n, int32_t k, int32_t len, int32_t min_votes,
                      int32_t P, uint32_t flags, double eps, double mo) {
        return tvz_align_parts_flags_shards(hs, n_shards, nullptr, nullptr, 1, len, nullptr, 1, 1, k, eps, mo, r, n, min_votes, P,
                                            flags, nullptr, nullptr, nullptr, 0, nullptr);
    };
    // everything wrong at once: the rate list speaks first, then min_votes, k, the query limit, max_parts, the flags, eps, B
    CHECK(call(bad_rates, 2, 0, 4096, 0, 5, 4u, 0.0, -1.0) == TVZ_ERR_INVALID && said("rate 1"));
    CHECK(call(rates, 0, 0, 4096, 0, 5, 4u, 0.0, -1.0) == TVZ_ERR_UNSUPPORTED && said("n_rates=0"));
    CHECK(call(rates, 2, 0, 4096, 0, 5, 4u, 0.0, -1.0) == TVZ_ERR_INVALID && said("min_votes 0"));
    CHECK(call(rates, 2, 0, 4096, 1, 5, 4u, 0.0, -1.0) == TVZ_ERR_UNSUPPORTED && said("k=0"));
    CHECK(call(rates, 2, 4, 4096, 1, 5, 4u, 0.0, -1.0) == TVZ_ERR_UNSUPPORTED && said("max_query_len 4096"));
    CHECK(call(rates, 2, 4, 10, 1, 5, 4u, 0.0, -1.0) == TVZ_ERR_UNSUPPORTED && said("max_parts=5"));
    CHECK(call(rates, 2, 4, 10, 1, 0, 4u, 0.0, -1.0) == TVZ_ERR_UNSUPPORTED && said("max_parts=0"));
    CHECK(call(rates, 2, 4, 10, 1, 2, 4u, 0.0, -1.0) == TVZ_ERR_INVALID && said("alignment parts: unknown flag bits 0x4"));
    CHECK(call(rates, 2, 4, 10, 1, 2, 9u, 1.0, 4194305.0) == TVZ_ERR_INVALID && said("unknown flag bits 0x1"));
    CHECK(call(rates, 2, 4, 10, 1, 2, 0x80000008u, 0.1, 1.0) == TVZ_ERR_INVALID && said("unknown flag bits 0x80000000"));
    CHECK(call(rates, 2, 4, 10, 1, 2, 1u, 0.1, 1.0) == TVZ_ERR_INVALID && said("unknown flag bits 0x1"));
    for (uint32_t ok : {0u, (uint32_t)TVZ_ALIGN_TWO_BINS}) {
        CHECK(call(rates, 2, 4, 10, 1, 2, ok, 0.0, 1.0) == TVZ_ERR_INVALID && said("eps must be > 0"));
        CHECK(call(rates, 2, 4, 10, 1, 2, ok, 0.1, -1.0) == TVZ_ERR_INVALID && !said("flag"));
        CHECK(call(rates, 2, 4, 10, 1, 2, ok, 1.0, 4194305.0) == TVZ_ERR_UNSUPPORTED && said("TVZ_ALIGN_WIDE_MAX_B"));
        CHECK(call(rates, 2, 4, 10, 1, 2, ok, 1.0, 4194304.0) == TVZ_ERR_INVALID && !said("flag"));      // good parameters: the NULL handle
    }
    // the call without flags says what it said
    CHECK(tvz_align_parts(nullptr, nullptr, nullptr, 1, 10, nullptr, 1, 1, 4, 0.0, 1.0, rates, 2, 1, 2, nullptr, nullptr, 0, nullptr) ==
              TVZ_ERR_INVALID && said("eps must be > 0"));
    // the _shards form: the same early checks in the same order, then its own
    tvz_corpus *none[2] = {nullptr, nullptr};
    CHECK(shards(nullptr, 17, rates, 2, 4, 10, 1, 5, 4u, 0.0, 1.0) == TVZ_ERR_UNSUPPORTED && said("max_parts=5"));
    CHECK(shards(nullptr, 17, rates, 2, 4, 10, 1, 2, 4u, 0.0, 1.0) == TVZ_ERR_INVALID && said("unknown flag bits 0x4"));
    CHECK(shards(nullptr, 17, rates, 2, 4, 10, 1, 2, 8u, 0.0, 1.0) == TVZ_ERR_INVALID && said("eps must be > 0"));
    CHECK(shards(nullptr, 17, rates, 2, 4, 10, 1, 2, 8u, 0.1, 1.0) == TVZ_ERR_INVALID && said("no shards"));
    CHECK(shards(none, 17, rates, 2, 4, 10, 1, 2, 8u, 0.1, 1.0) == TVZ_ERR_UNSUPPORTED && said("17 lists"));
    CHECK(shards(none, 2, rates, 2, 4, 10, 1, 2, 8u, 0.1, 1.0) == TVZ_ERR_INVALID && said("shard 0 is NULL"));
    // ---- the carving, as it was
    for (size_t mis : {(size_t)0, (size_t)8, (size_t)248})
        for (int32_t Q : {1, 3, 64})
            for (int32_t k : {1, 5, 64})
                for (int32_t max_parts = 1; max_parts <= TVZ_ALIGN_MAX_PARTS; ++max_parts) {
                    carve(Q, 40, 0, k, max_parts, mis);
                    carve(Q, 4095, (int64_t)Q * 100 + 4095, k, max_parts, mis);
                }
    std::printf(g_bad ? "FAILED %d\n" : "HOST_OK\n", g_bad);
    return g_bad ? 1 : 0;
}
