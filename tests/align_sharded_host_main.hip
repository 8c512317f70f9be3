// Stand-alone host program (its own main) for tests/test_align_topk_sharded_host_cpu.py: the sizing and carving code of
// the alignment top-k - every form of the table, plain and sharded, one layout -, built for the HOST only with
// -fsanitize=address,undefined and run without a GPU.  It includes the library's translation unit, so the functions
// under test are the product's own, not copies.
//   - walks align_topk_ws_layout + tol_ws_layout over a real host buffer at aligned and misaligned bases, for the four
//     forms and the sharded forms of the first two: every region lies inside the buffer of the sizing function's byte
//     count, in order, none overlapping, and is written to its end - so each sizing export equals the walk;
//   - the exported sizing functions: the sharded size = the plain one + the blocks, monotone in every argument;
//   - the refusals of the new entry points that return before any HIP call.
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

// the form's sizing export for this many ranks (0: the plain call); only the first two forms have a sharded one
size_t sized(AlignForm form, int32_t Q, int32_t max_len, int64_t keys, int32_t k, int32_t n_ranks) {
    switch (form) {
    case kAlignBounded:
        return n_ranks ? tvz_align_topk_sharded_workspace_bytes(Q, max_len, keys, k, n_ranks)
                       : tvz_align_topk_workspace_bytes(Q, max_len, keys, k);
    case kAlignWide:
        return n_ranks ? tvz_align_wide_topk_sharded_workspace_bytes(Q, max_len, keys, k, n_ranks)
                       : tvz_align_wide_topk_workspace_bytes(Q, max_len, keys, k);
    case kAlignRates: return tvz_align_rates_topk_workspace_bytes(Q, max_len, keys, k);
    default: return tvz_align_span_topk_workspace_bytes(Q, max_len, keys, k);
    }
}

void carve(AlignForm form, int32_t Q, int32_t max_len, int64_t keys, int32_t k, int32_t n_ranks, size_t misalign) {
    const AlignTopkForm &f = kAlignForms[form];
    const size_t need = sized(form, Q, max_len, keys, k, n_ranks);
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
    for (int i = 0; i < 4; ++i) {    // the form's uint32 lists and no others: a kept hit is 16 + 4 * part32 bytes
        CHECK((w.part32[i] != nullptr) == (i < f.part32));
        if (w.part32[i]) r.push_back({(unsigned char *)w.part32[i], lists * 4});
    }
    if (n_ranks) {
        CHECK(w.local != nullptr && w.gathered != nullptr);
        r.push_back({(unsigned char *)w.local, block});
        r.push_back({(unsigned char *)w.gathered, (size_t)n_ranks * block});
    } else {
        CHECK(w.local == nullptr && w.gathered == nullptr);
    }
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
                for (int form = 0; form < kAlignFormCount; ++form)
                    for (int32_t n_ranks : {0, 1, 3, 16}) {
                        if (n_ranks && !kAlignForms[form].sharded_sizer) continue;      // (no RCCL form: nothing to size)
                        carve((AlignForm)form, Q, 40, 0, k, n_ranks, mis);
                        carve((AlignForm)form, Q, 4095, (int64_t)Q * 100 + 4095, k, n_ranks, mis);
                    }
    // the table's arithmetic: bytes per kept hit, and only the first two forms are sharded
    CHECK(kAlignForms[kAlignBounded].part32 == 0 && kAlignForms[kAlignWide].part32 == 1);
    CHECK(kAlignForms[kAlignRates].part32 == 2 && kAlignForms[kAlignSpan].part32 == 4);
    CHECK(kAlignForms[kAlignRates].cols == 5 && kAlignForms[kAlignSpan].cols == 8);
    CHECK(kAlignForms[kAlignRates].sharded_sizer == nullptr && kAlignForms[kAlignSpan].sharded_sizer == nullptr);
    // the sharded size: the plain one + local and gathered blocks, each rounded to 256 bytes; monotone
    for (int32_t Q : {0, 1, 2, 7, 64})
        for (int32_t len : {0, 1, 40, 4095})
            for (int32_t k : {1, 2, 16, 64})
                for (int32_t n : {0, 1, 2, 8, 16}) {
                    const size_t plain = tvz_align_topk_workspace_bytes(Q, len, 0, k);
                    const size_t sh = tvz_align_topk_sharded_workspace_bytes(Q, len, 0, k, n);
                    const size_t blocks = (size_t)(1 + std::max(n, 1)) * Q * (k + 1) * 16;
                    CHECK(sh >= plain + blocks && sh <= plain + blocks + 2 * 256);
                    CHECK(tvz_align_topk_sharded_workspace_bytes(Q + 1, len, 0, k, n) >= sh);
                    CHECK(tvz_align_topk_sharded_workspace_bytes(Q, len + 1, 0, k, n) >= sh);
                    CHECK(k == 64 || tvz_align_topk_sharded_workspace_bytes(Q, len, 0, k + 1, n) >= sh);
                    CHECK(tvz_align_topk_sharded_workspace_bytes(Q, len, 0, k, n + 1) >= sh);
                    CHECK(tvz_align_topk_sharded_workspace_bytes(Q, len, (int64_t)Q * len + 100, k, n) >= sh);
                }
    CHECK(tvz_align_topk_sharded_workspace_bytes(-1, 1, 0, 1, 1) == 0 && tvz_align_topk_sharded_workspace_bytes(1, 1, 0, 0, 1) == 0);
    CHECK(tvz_align_topk_sharded_workspace_bytes(1, 1, 0, 1, -1) == 0 && tvz_align_topk_sharded_workspace_bytes(1, 1, -1, 1, 1) == 0);
    // refusals that return before any HIP call
    alignas(16) int32_t i4[64] = {};
    double d = 0.0;
    int64_t off[2] = {0, 1};
    CHECK(tvz_align_topk_merge(i4, 17, 1, 4, &d, off, i4, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_topk_merge(i4, 0, 1, 4, &d, off, i4, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_topk_merge(i4, 2, 1, 65, &d, off, i4, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_topk_merge(i4, 2, -1, 4, &d, off, i4, i4, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_topk_merge(nullptr, 2, 1, 4, &d, off, i4, i4, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_topk_merge(i4, 2, 1, 4, &d, off, i4 + 1, i4, nullptr) == TVZ_ERR_INVALID);      // d_topk misaligned
    CHECK(tvz_align_topk_merge(i4, 2, 0, 4, nullptr, nullptr, nullptr, nullptr, nullptr) == TVZ_OK);
    CHECK(tvz_align_topk_shards(nullptr, 1, &d, off, 1, 1, 0.1, 1.0, 1, 0, nullptr, 4, i4, i4, i4, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    tvz_corpus *none[1] = {nullptr};
    CHECK(tvz_align_topk_shards(none, 1, &d, off, 1, 1, 0.1, 1.0, 1, 0, nullptr, 4, i4, i4, i4, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    CHECK(tvz_align_topk_shards(none, 17, &d, off, 1, 1, 0.1, 1.0, 1, 0, nullptr, 4, i4, i4, i4, nullptr, 0, nullptr) == TVZ_ERR_UNSUPPORTED);
    std::printf(g_bad ? "FAILED %d\n" : "HOST_OK\n", g_bad);
    return g_bad ? 1 : 0;
}
