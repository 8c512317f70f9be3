// Stand-alone host program (its own main) for tests/test_align_two_bins_host_cpu.py: the host code TVZ_ALIGN_TWO_BINS
// touched - the permitted-flags column of kAlignForms and check_align_flags, the refusals of the three calls, their
// _shards forms and their merges that return before any HIP call, and the sizing exports, which no flag reaches -
// built for the HOST only with -fsanitize=address,undefined and run without a GPU.  It includes the library's
// translation unit, so the functions under test are the product's own, not copies.
#include <cstdio>
#include <cstring>

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

bool said(const char *word) { return std::strstr(tvz_last_error(), word) != nullptr; }

void the_table() {
    CHECK(TVZ_ALIGN_TWO_BINS == 8u && kAlTwoBins == TVZ_ALIGN_TWO_BINS);
    CHECK(kAlignForms[kAlignBounded].flags == 0u);
    CHECK(kAlignForms[kAlignWide].flags == (TVZ_ALIGN_CONTAIN | TVZ_ALIGN_TWO_BINS));
    CHECK(kAlignForms[kAlignRates].flags == (TVZ_ALIGN_CONTAIN | TVZ_ALIGN_TWO_BINS));
    CHECK(kAlignForms[kAlignSpan].flags == (TVZ_ALIGN_CONTAIN | TVZ_ALIGN_LOCAL | TVZ_ALIGN_TWO_BINS));
    CHECK(kAlignForms[kAlignSpan].exclusive == (TVZ_ALIGN_CONTAIN | TVZ_ALIGN_LOCAL));      // the bit is no score kind
    const AlignForm forms[] = {kAlignWide, kAlignRates, kAlignSpan};
    for (AlignForm form : forms) {
        const AlignTopkForm &f = kAlignForms[form];
        for (uint32_t flags = 0; flags < 32u; ++flags) {
            const bool known = (flags & ~f.flags) == 0u;
            const bool both = f.exclusive != 0u && (flags & f.exclusive) == f.exclusive;
            for (const char *where : {"", " merge"}) {
                const int rc = check_align_flags(f, flags, where);
                CHECK(rc == (known && !both ? TVZ_OK : TVZ_ERR_INVALID));
                if (!known) CHECK(said("unknown flag bits"));
                else if (both) CHECK(said("two score kinds"));
            }
        }
        CHECK(check_align_flags(f, 4u, "") == TVZ_ERR_INVALID && said("unknown flag bits 0x4"));
        CHECK(check_align_flags(f, 8u | 4u, "") == TVZ_ERR_INVALID && said("unknown flag bits 0x4"));
        CHECK(check_align_flags(f, 0x80000008u, "") == TVZ_ERR_INVALID && said("unknown flag bits 0x80000000"));
    }
    CHECK(check_align_flags(kAlignForms[kAlignBounded], 8u, "") == TVZ_ERR_INVALID);
}

void the_exports() {
    double rates[2] = {1.0, 0.96};
    alignas(16) int32_t i4[4] = {0, 0, 0, 0};
    // the span form refuses its flags before it looks at the handle; 8, 8|1, 8|2 get past that to the NULL handle
    for (uint32_t flags : {8u, 9u, 10u}) {
        CHECK(tvz_align_span_topk(nullptr, nullptr, nullptr, 1, 4, 1.0 / 30, 1.0, rates, 2, 1, 0, flags, nullptr, 16, nullptr,
                                  nullptr, 0, nullptr) == TVZ_ERR_INVALID);
        CHECK(!said("flag") && !said("TVZ_ALIGN"));
        CHECK(tvz_align_span_topk_shards(nullptr, 1, nullptr, nullptr, 1, 4, 1.0 / 30, 1.0, rates, 2, 1, 0, flags, nullptr, 16,
                                         nullptr, nullptr, nullptr, nullptr, 0, nullptr) == TVZ_ERR_INVALID);
        CHECK(!said("flag") && !said("TVZ_ALIGN"));
    }
    for (uint32_t flags : {11u, 4u, 12u, 0x80000008u}) {
        CHECK(tvz_align_span_topk(nullptr, nullptr, nullptr, 1, 4, 1.0 / 30, 1.0, rates, 2, 1, 0, flags, nullptr, 16, nullptr,
                                  nullptr, 0, nullptr) == TVZ_ERR_INVALID);
        CHECK(flags == 11u ? said("two score kinds") : said("unknown flag bits"));
    }
    // the wide and rates forms look at the handle first: INVALID either way
    for (uint32_t flags : {8u, 9u, 11u, 4u, 12u, 0x80000008u, 2u, 10u}) {
        CHECK(tvz_align_wide_topk(nullptr, nullptr, nullptr, 1, 4, 1.0 / 30, 1.0, 1, 0, flags, nullptr, 16, nullptr, nullptr, 0,
                                  nullptr) == TVZ_ERR_INVALID);
        CHECK(tvz_align_rates_topk(nullptr, nullptr, nullptr, 1, 4, 1.0 / 30, 1.0, rates, 2, 1, 0, flags, nullptr, 16, nullptr,
                                   nullptr, 0, nullptr) == TVZ_ERR_INVALID);
    }
    // the merges: Q = 0 returns behind the flag check and in front of any launch
    for (uint32_t flags : {0u, 1u, 8u, 9u}) {
        CHECK(tvz_align_wide_topk_merge(i4, 3, 0, 4, flags, nullptr, nullptr, i4, i4, nullptr) == TVZ_OK);
        CHECK(tvz_align_rates_topk_merge(i4, 3, 0, 4, flags, nullptr, nullptr, i4, i4, nullptr) == TVZ_OK);
    }
    for (uint32_t flags : {0u, 1u, 2u, 8u, 9u, 10u})
        CHECK(tvz_align_span_topk_merge(i4, 3, 0, 4, flags, nullptr, nullptr, i4, i4, nullptr) == TVZ_OK);
    for (uint32_t flags : {2u, 10u, 4u, 12u, 0x80000008u}) {
        CHECK(tvz_align_wide_topk_merge(i4, 3, 0, 4, flags, nullptr, nullptr, i4, i4, nullptr) == TVZ_ERR_INVALID);
        CHECK(said("merge: unknown flag bits"));
        CHECK(tvz_align_rates_topk_merge(i4, 3, 0, 4, flags, nullptr, nullptr, i4, i4, nullptr) == TVZ_ERR_INVALID);
    }
    for (uint32_t flags : {3u, 11u, 4u, 12u, 0x80000008u})
        CHECK(tvz_align_span_topk_merge(i4, 3, 0, 4, flags, nullptr, nullptr, i4, i4, nullptr) == TVZ_ERR_INVALID);
    // what the merges refused before the flags they still refuse with the bit set
    CHECK(tvz_align_wide_topk_merge(i4, 17, 0, 4, 8u, nullptr, nullptr, i4, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    CHECK(tvz_align_span_topk_merge(i4, 3, 0, 65, 8u, nullptr, nullptr, i4, i4, nullptr) == TVZ_ERR_UNSUPPORTED);
    // no sizing function takes flags: the pinned sizes (tests/golden/align_workspace_sizes.json) are every call's
    CHECK(tvz_align_wide_topk_workspace_bytes(1, 200, 0, 16) > 0 && tvz_align_span_topk_workspace_bytes(64, 4095, 0, 64) > 0);
    CHECK(tvz_version() == 404);
}

}  // namespace

int main() {
    the_table();
    the_exports();
    if (g_bad) {
        std::fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    std::puts("HOST_OK");
    return 0;
}
