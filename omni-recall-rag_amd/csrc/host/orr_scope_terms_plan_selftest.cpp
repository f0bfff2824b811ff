// orr_scope_terms_plan_selftest -- the rules of orr_scope_terms_plan.h on the CPU (no HIP, no GPU): the fold of 1, 2, 7 and 256
// terms' words for ALL and ANY against a bit-by-bit restatement, the tail mask at every kind of last word and in the padding
// words, and the validity of mode, term count and term offsets.
// Exit status 0 and a last line "orr_scope_terms_plan_selftest: ok" when everything holds; tests/test_scope_terms_cpu.py runs it.
#include <cstdio>
#include <random>
#include <vector>

#include "../orr_scope_terms_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static int64_t words_for(int64_t rows) { return ((rows + 31) / 32 + 3) / 4 * 4; }

// a row at a time: row 32 w + b is in iff it is a row of the shard and all / any of the terms hold its bit
static uint32_t word_by_bits(const std::vector<uint32_t> &tw, int32_t mode, int64_t w, int64_t n_rows)
{
    uint32_t out = 0;
    for (int b = 0; b < 32; ++b) {
        if (w * 32 + b >= n_rows) continue;
        size_t held = 0;
        for (uint32_t x : tw) held += (x >> b) & 1u;
        const bool in = mode == scope_terms::All ? held == tw.size() : held > 0;
        out |= (uint32_t)in << b;
    }
    return out;
}

static void test_fold()
{
    std::mt19937 rng(17);
    for (int32_t n : {1, 2, 7, 256})
        for (int rep = 0; rep < 300; ++rep) {
            std::vector<uint32_t> tw((size_t)n);
            // dense words for ALL to leave something, sparse ones for ANY to leave something out, plain random ones, and the extremes
            for (auto &x : tw) {
                const uint32_t a = rng(), b = rng(), c = rng();
                x = rep % 4 == 0 ? (a | b | c) : rep % 4 == 1 ? (a & b & c) : rep % 4 == 2 ? a : (rep & 4 ? 0xFFFFFFFFu : 0u);
            }
            if (rep % 7 == 3) tw[(size_t)(rng() % (uint32_t)n)] = 0u;            // a term that matched nothing
            if (rep % 7 == 5 && n > 1) tw[1] = tw[0];                            // the same term twice
            for (int32_t mode : {(int32_t)scope_terms::All, (int32_t)scope_terms::Any}) {
                CHECK(scope_terms::scope_word(tw.data(), n, mode, 0, 1 << 20) == word_by_bits(tw, mode, 0, 1 << 20));
                uint32_t acc = scope_terms::fold_identity(mode);
                for (uint32_t x : tw) acc = scope_terms::fold_word(acc, x, mode);
                CHECK(acc == word_by_bits(tw, mode, 0, 1 << 20));
            }
        }
    CHECK(scope_terms::fold_identity(scope_terms::All) == 0xFFFFFFFFu && scope_terms::fold_identity(scope_terms::Any) == 0u);
    // a term without a match empties ALL and adds nothing to ANY
    const uint32_t two[2] = {0xF0F0F0F0u, 0u};
    CHECK(scope_terms::scope_word(two, 2, scope_terms::All, 0, 64) == 0u);
    CHECK(scope_terms::scope_word(two, 2, scope_terms::Any, 0, 64) == 0xF0F0F0F0u);
}

static void test_tail_mask()
{
    std::mt19937 rng(23);
    for (int64_t n_rows : {1ll, 31ll, 32ll, 33ll, 63ll, 64ll, 127ll, 128ll, 129ll, 70001ll, 200000ll, 196608ll, 1000001ll}) {
        const int64_t words = words_for(n_rows);
        CHECK(words % 4 == 0 && words * 32 >= n_rows);
        for (int64_t w = 0; w < words; ++w) {
            uint32_t want = 0;
            for (int b = 0; b < 32; ++b)
                if (w * 32 + b < n_rows) want |= 1u << b;
            if (scope_terms::tail_mask(w, n_rows) != want) { CHECK(!"tail_mask differs from the row-by-row mask"); break; }
        }
        // n_rows % 32 in {0, 1, 31} are all in the list above; the last word with rows, and every padding word behind it, for both
        // modes with all-ones term words (bitmaps with junk in their tails: what the mask is there for)
        const int64_t last = (n_rows - 1) / 32;
        const std::vector<uint32_t> ones(3, 0xFFFFFFFFu);
        for (int32_t mode : {(int32_t)scope_terms::All, (int32_t)scope_terms::Any}) {
            CHECK(scope_terms::scope_word(ones.data(), 3, mode, last, n_rows) == word_by_bits(ones, mode, last, n_rows));
            const int rem = (int)(n_rows % 32);
            CHECK(scope_terms::scope_word(ones.data(), 3, mode, last, n_rows) == (rem == 0 ? 0xFFFFFFFFu : (1u << rem) - 1u));
            for (int64_t w = last + 1; w < words; ++w) CHECK(scope_terms::scope_word(ones.data(), 3, mode, w, n_rows) == 0u);
            if (last > 0) CHECK(scope_terms::scope_word(ones.data(), 3, mode, last - 1, n_rows) == 0xFFFFFFFFu);
        }
        // random words in the last word
        for (int rep = 0; rep < 50; ++rep) {
            const std::vector<uint32_t> tw = {(uint32_t)rng(), (uint32_t)rng() | (uint32_t)rng()};
            for (int32_t mode : {(int32_t)scope_terms::All, (int32_t)scope_terms::Any})
                CHECK(scope_terms::scope_word(tw.data(), 2, mode, last, n_rows) == word_by_bits(tw, mode, last, n_rows));
        }
    }
    CHECK(scope_terms::tail_mask(0, 0) == 0u && scope_terms::tail_mask(3, 0) == 0u);
}

static void test_arguments()
{
    CHECK(scope_terms::mode_valid(0) && scope_terms::mode_valid(1) && !scope_terms::mode_valid(-1) && !scope_terms::mode_valid(2));
    CHECK(scope_terms::All == 0 && scope_terms::Any == 1);
    CHECK(scope_terms::terms_valid(0) && scope_terms::terms_valid(1) && scope_terms::terms_valid(256));
    CHECK(!scope_terms::terms_valid(-1) && !scope_terms::terms_valid(257));
    const uint32_t good[4] = {0, 2, 5, 6}, empty_mid[4] = {0, 2, 2, 6}, empty_first[3] = {4, 4, 6}, back[4] = {0, 5, 3, 6};
    CHECK(scope_terms::first_bad_term(good, 3) == -1);
    CHECK(scope_terms::first_bad_term(good, 0) == -1);
    CHECK(scope_terms::first_bad_term(empty_mid, 3) == 1);
    CHECK(scope_terms::first_bad_term(empty_first, 2) == 0);
    CHECK(scope_terms::first_bad_term(back, 3) == 1);
}

int main()
{
    test_fold();
    test_tail_mask();
    test_arguments();
    if (g_failed) { printf("orr_scope_terms_plan_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("orr_scope_terms_plan_selftest: ok\n");
    return 0;
}
