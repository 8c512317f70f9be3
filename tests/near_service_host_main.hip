// Stand-alone host program (its own main) for tests/test_near_service_host_cpu.py: the sizing and carving code of the
// workspaces this library's sharded near-duplicate calls added - the alignment top-k with rates and with spans with
// their local and gathered blocks, and the parts call with its local and gathered answers -, built for the HOST only with
// -fsanitize=address,undefined and run without a GPU.  It includes the library's translation unit, so the functions under
// test are the product's own, not copies.
//   - walks align_topk_ws_layout / align_parts_ws_layout + tol_ws_layout over a real host buffer at aligned and misaligned
//     bases: every region lies inside the buffer of the sharded sizing function's byte count, in order, none overlapping,
//     and is written to its end - so each sizing export equals the walk;
//   - the exported sizing functions: the sharded size = the plain one + the blocks, monotone in every argument, 0 where
//     the plain one is 0;
//   - the refusals of tvz_align_parts_merge and tvz_align_parts_shards that return before any HIP call.
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

// the regions in the order they were carved: inside [base, base + need), 256-byte aligned, disjoint; each is written
void written_in_order(const std::vector<Region> &r, unsigned char *base, size_t need) {
    unsigned char *at = base;
    for (const Region &x : r) {
        CHECK(x.p >= at && ((uintptr_t)x.p & 255) == 0 && x.p + x.bytes <= base + need);
        if (x.p >= at && x.p + x.bytes <= base + need) memset(x.p, 0x5a, x.bytes);     // (ASan watches the vector's end)
        at = x.p + x.bytes;
    }
}

void push_sorted_queries(std::vector<Region> &r, Carver &cv, int32_t Q, int64_t room) {
    const TolWs t = tol_ws_layout(cv, Q, room);
    r.push_back({(unsigned char *)t.qm, (size_t)Q * 4});
    r.push_back({(unsigned char *)t.sv, (size_t)room * 8});
    r.push_back({(unsigned char *)t.sp, (size_t)room * 4});
}

void carve_form(AlignForm form, int32_t Q, int32_t max_len, int64_t keys, int32_t k, int32_t n_ranks, size_t misalign) {
    const AlignTopkForm &f = kAlignForms[form];
    const size_t need = form == kAlignRates ? tvz_align_rates_topk_sharded_workspace_bytes(Q, max_len, keys, k, n_ranks)
                                            : tvz_align_span_topk_sharded_workspace_bytes(Q, max_len, keys, k, n_ranks);
    CHECK(need > 0);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *base = buf.data() + misalign;
    Carver cv(base);
    const AlignTopkWs w = align_topk_ws_layout(cv, f, Q, k, n_ranks);
    {   // the sizing export is the same walk from NULL, + the sorted queries' part
        Carver from_null(nullptr);
        align_topk_ws_layout(from_null, f, Q, k, n_ranks);
        CHECK(need == from_null.fixed() + tol_ws_bytes(Q, std::max<int64_t>(keys > 0 ? keys : (int64_t)Q * max_len, max_len)));
    }
    const int64_t room = tol_ws_room(Q, need - cv.fixed());
    CHECK(room >= std::max<int64_t>(keys, max_len));
    const size_t lists = (size_t)tol_topk_max_lists(Q) * (size_t)k, block = (size_t)Q * (size_t)(k + 1) * 4 * f.cols;
    std::vector<Region> r = {{(unsigned char *)w.totals, (size_t)Q * 4}, {(unsigned char *)w.part_w, lists * 8},
                             {(unsigned char *)w.part_p, lists * 8}};
    for (int i = 0; i < f.part32; ++i) r.push_back({(unsigned char *)w.part32[i], lists * 4});
    CHECK(w.local != nullptr && w.gathered != nullptr);
    r.push_back({(unsigned char *)w.local, block});
    r.push_back({(unsigned char *)w.gathered, (size_t)n_ranks * block});
    push_sorted_queries(r, cv, Q, room);
    written_in_order(r, base, need);
}

void carve_parts(int32_t Q, int32_t max_len, int64_t keys, int32_t k, int32_t max_parts, int32_t n_ranks, size_t misalign) {
    const size_t need = tvz_align_parts_sharded_workspace_bytes(Q, max_len, keys, k, max_parts, n_ranks);
    CHECK(need > 0);
    std::vector<unsigned char> buf(need + 512);
    unsigned char *base = buf.data() + misalign;
    Carver cv(base);
    const AlignPartsWs w = align_parts_ws_layout(cv, Q, k, max_parts, n_ranks);
    {
        Carver from_null(nullptr);
        align_parts_ws_layout(from_null, Q, k, max_parts, n_ranks);
        CHECK(need == from_null.fixed() + tol_ws_bytes(Q, std::max<int64_t>(keys > 0 ? keys : (int64_t)Q * max_len, max_len)));
    }
    const int64_t room = tol_ws_room(Q, need - cv.fixed());
    CHECK(room >= std::max<int64_t>(keys, max_len));
    const size_t pairs = (size_t)Q * (size_t)k, answer = pairs * (size_t)(1 + max_parts) * 24;
    std::vector<Region> r = {{(unsigned char *)w.counts, pairs * 4},
                             {(unsigned char *)w.slots, pairs * TVZ_ALIGN_PARTS_MAX_ROWS * 8},
                             {(unsigned char *)w.scratch, TVZ_ALIGN_PARTS_MAX_ROWS * answer}};
    CHECK(w.local != nullptr && w.gathered != nullptr);
    r.push_back({(unsigned char *)w.local, answer});
    r.push_back({(unsigned char *)w.gathered, (size_t)n_ranks * answer});
    push_sorted_queries(r, cv, Q, room);
    written_in_order(r, base, need);
}

}  // namespace

int main() {
    for (size_t mis : {(size_t)0, (size_t)8, (size_t)248})
        for (int32_t Q : {1, 3, 64})
            for (int32_t k : {1, 5, 64})
                for (int32_t n_ranks : {1, 3, 16}) {
                    for (AlignForm form : {kAlignRates, kAlignSpan}) {
                        carve_form(form, Q, 40, 0, k, n_ranks, mis);
                        carve_form(form, Q, 4095, (int64_t)Q * 100 + 4095, k, n_ranks, mis);
                    }
                    for (int32_t max_parts : {1, 4}) {
                        carve_parts(Q, 40, 0, k, max_parts, n_ranks, mis);
                        carve_parts(Q, 4095, (int64_t)Q * 100 + 4095, k, max_parts, n_ranks, mis);
                    }
                }
    // the plain parts call and its _shards form carve no blocks
    {
        Carver cv(nullptr);
        const AlignPartsWs w = align_parts_ws_layout(cv, 3, 5, 2);
        CHECK(w.local == nullptr && w.gathered == nullptr);
    }
    // the sharded sizes: the plain one + local and gathered blocks, each rounded to 256 bytes; monotone; 0 where the plain
    // one is 0 and for a negative rank count
    for (int32_t Q : {0, 1, 2, 7, 64})
        for (int32_t len : {0, 1, 40, 4095})
            for (int32_t k : {1, 2, 16, 64})
                for (int32_t n : {0, 1, 2, 8, 16}) {
                    const size_t blocks = (size_t)(1 + std::max(n, 1)) * Q * (k + 1);
                    const size_t rates = tvz_align_rates_topk_sharded_workspace_bytes(Q, len, 0, k, n);
                    const size_t span = tvz_align_span_topk_sharded_workspace_bytes(Q, len, 0, k, n);
                    const size_t r0 = tvz_align_rates_topk_workspace_bytes(Q, len, 0, k), s0 = tvz_align_span_topk_workspace_bytes(Q, len, 0, k);
                    CHECK(rates >= r0 + blocks * 20 && rates <= r0 + blocks * 20 + 2 * 256);
                    CHECK(span >= s0 + blocks * 32 && span <= s0 + blocks * 32 + 2 * 256);
                    CHECK(tvz_align_span_topk_sharded_workspace_bytes(Q + 1, len, 0, k, n) >= span);
                    CHECK(tvz_align_span_topk_sharded_workspace_bytes(Q, len + 1, 0, k, n) >= span);
                    CHECK(k == 64 || tvz_align_span_topk_sharded_workspace_bytes(Q, len, 0, k + 1, n) >= span);
                    CHECK(tvz_align_span_topk_sharded_workspace_bytes(Q, len, 0, k, n + 1) >= span);
                    CHECK(tvz_align_rates_topk_sharded_workspace_bytes(Q, len, (int64_t)Q * len + 100, k, n) >= rates);
                    for (int32_t P : {1, 2, 4}) {
                        const size_t p0 = tvz_align_parts_workspace_bytes(Q, len, 0, k, P);
                        const size_t sz = tvz_align_parts_sharded_workspace_bytes(Q, len, 0, k, P, n);
                        const size_t answers = (size_t)(1 + std::max(n, 1)) * Q * k * (size_t)(1 + P) * 24;
                        CHECK(sz >= p0 + answers && sz <= p0 + answers + 2 * 256);
                        CHECK(tvz_align_parts_sharded_workspace_bytes(Q + 1, len, 0, k, P, n) >= sz);
                        CHECK(tvz_align_parts_sharded_workspace_bytes(Q, len, 0, k, P, n + 1) >= sz);
                        CHECK(P == 4 || tvz_align_parts_sharded_workspace_bytes(Q, len, 0, k, P + 1, n) >= sz);
                    }
                }
    CHECK(tvz_align_rates_topk_sharded_workspace_bytes(-1, 1, 0, 1, 1) == 0 && tvz_align_span_topk_sharded_workspace_bytes(1, 1, 0, 0, 1) == 0);
    CHECK(tvz_align_rates_topk_sharded_workspace_bytes(1, 1, 0, 1, -1) == 0 && tvz_align_span_topk_sharded_workspace_bytes(1, 1, -1, 1, 1) == 0);
    CHECK(tvz_align_parts_sharded_workspace_bytes(1, 1, 0, 1, 0, 1) == 0 && tvz_align_parts_sharded_workspace_bytes(1, 1, 0, 1, 5, 1) == 0);
    CHECK(tvz_align_parts_sharded_workspace_bytes(1, 1, 0, 1, 1, -1) == 0 && tvz_align_parts_sharded_workspace_bytes(-1, 1, 0, 1, 1, 1) == 0);
    // refusals that return before any HIP call
    int32_t i4[64] = {};
    double d = 0.0;
    int64_t off[2] = {0, 1};
    const double rates[1] = {1.0};
    CHECK(tvz_align_parts_merge(i4, 0, 1, 1, 1, i4, nullptr) == TVZ_ERR_UNSUPPORTED && tvz_align_parts_merge(i4, 17, 1, 1, 1, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_parts_merge(i4, 2, 1, 0, 1, i4, nullptr) == TVZ_ERR_UNSUPPORTED && tvz_align_parts_merge(i4, 2, 1, 65, 1, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_parts_merge(i4, 2, 1, 1, 0, i4, nullptr) == TVZ_ERR_UNSUPPORTED && tvz_align_parts_merge(i4, 2, 1, 1, 5, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_parts_merge(i4, 2, -1, 1, 1, i4, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_parts_merge(nullptr, 2, 1, 1, 1, i4, nullptr) == TVZ_ERR_INVALID && tvz_align_parts_merge(i4, 2, 1, 1, 1, nullptr, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_parts_merge(nullptr, 2, 0, 1, 1, nullptr, nullptr) == TVZ_OK);
    tvz_corpus *none[1] = {nullptr};
    auto shards = [&](tvz_corpus *const *h, int32_t n, const double *r, int32_t n_rates, int32_t P) {
        return tvz_align_parts_shards(h, n, &d, off, 1, 1, i4, 1, 1, 1, 0.1, 1.0, r, n_rates, 1, P, i4, i4, nullptr, 0, nullptr);
    };
    CHECK(shards(nullptr, 1, rates, 1, 2) == TVZ_ERR_INVALID && shards(none, 1, rates, 1, 2) == TVZ_ERR_INVALID);
    CHECK(shards(none, 17, rates, 1, 2) == TVZ_ERR_UNSUPPORTED && shards(none, 0, rates, 1, 2) == TVZ_ERR_INVALID);
    CHECK(shards(none, 17, rates, 0, 2) == TVZ_ERR_UNSUPPORTED && shards(none, 1, nullptr, 1, 2) == TVZ_ERR_INVALID);     // the rate list first
    CHECK(shards(none, 1, rates, 1, 5) == TVZ_ERR_UNSUPPORTED);                                                          // ... then max_parts
    std::printf(g_bad ? "FAILED %d\n" : "HOST_OK\n", g_bad);
    return g_bad ? 1 : 0;
}
