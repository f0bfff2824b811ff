// orr_scope_plan_selftest -- the rules of orr_scope_plan.h on the CPU (no HIP, no GPU): form choice, the ladder's end, slices
// that cover every query exactly once within the budget, offset validation, and the bitmap clip against a scalar restatement.
// Exit status 0 and a last line "orr_scope_plan_selftest: ok" when everything holds; tests/test_scope_plan_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../orr_scope_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

using scope::Form;
using scope::Rung;

static void test_form_choice()
{
    // the default k of 10 over a scope of thousands: one selection list's worth of records, as an unscoped search starts
    Rung r = scope::first_rung(10, 2000, 64);
    CHECK(r.form == Form::Selection && r.kprime == 32);
    // k' would exceed a selection list
    r = scope::first_rung(65, 5000, 64);
    CHECK(r.form == Form::AllRecords && r.kprime == 5000);
    r = scope::first_rung(200, 5000, 64);
    CHECK(r.form == Form::AllRecords && r.kprime == 5000);
    // k' already covers every query's scope
    r = scope::first_rung(10, 32, 64);
    CHECK(r.form == Form::AllRecords && r.kprime == 32);
    r = scope::first_rung(10, 1, 64);
    CHECK(r.form == Form::AllRecords && r.kprime == 1);
    r = scope::first_rung(10, 33, 64);
    CHECK(r.form == Form::Selection && r.kprime == 32);
    // k up to 56 still fits one list with its margin
    r = scope::first_rung(56, 100000, 64);
    CHECK(r.form == Form::Selection && r.kprime == 64);
    r = scope::first_rung(57, 100000, 64);
    CHECK(r.form == Form::AllRecords);
    // an empty batch of scopes still names a form with k' >= 1 (the records' array has a size)
    r = scope::first_rung(10, 0, 64);
    CHECK(r.form == Form::AllRecords && r.kprime == 1);
}

static void test_ladder_ends()
{
    for (int32_t take : {1, 5, 10, 42, 56, 57, 64, 65, 200, 1000})
        for (int64_t max_scope : {0ll, 1ll, 2ll, 31ll, 32ll, 33ll, 64ll, 65ll, 300ll, 100000ll, 1ll << 40}) {
            Rung r = scope::first_rung(take, max_scope, 64);
            int steps = 0;
            int64_t last_k = 0;
            bool saw_all = false;
            while (r.form != Form::Done) {
                CHECK(r.kprime >= 1);
                CHECK(!saw_all);                                       // AllRecords is the end
                if (r.form == Form::Selection) {
                    CHECK(r.kprime <= 64 && r.kprime < max_scope);     // a selection always leaves rows out: else AllRecords
                    CHECK(r.kprime > last_k);
                    last_k = r.kprime;
                } else {
                    CHECK(r.kprime == std::max<int64_t>(1, max_scope)); // every scoped row a record
                    saw_all = true;
                }
                r = scope::next_rung(r, max_scope, 64);
                CHECK(++steps <= scope::kMaxRungs);
                if (steps > scope::kMaxRungs) break;
            }
            CHECK(saw_all);                                            // every ladder reaches the certified-by-construction form
        }
    Rung r = scope::next_rung(Rung{Form::Selection, 4}, 1000, 64);
    CHECK(r.form == Form::Selection && r.kprime == 16);
    r = scope::next_rung(Rung{Form::Selection, 32}, 1000, 64);
    CHECK(r.form == Form::AllRecords && r.kprime == 1000);
    r = scope::next_rung(Rung{Form::Selection, 8}, 20, 64);
    CHECK(r.form == Form::AllRecords && r.kprime == 20);
}

static void test_slices()
{
    std::mt19937_64 rng(7);
    for (int round = 0; round < 400; ++round) {
        const int32_t n = 1 + (int32_t)(rng() % 300);
        std::vector<uint32_t> counts((size_t)n);
        const uint32_t top = round % 3 == 0 ? 100u : round % 3 == 1 ? 40000u : 3000000u;
        for (auto &c : counts) c = (uint32_t)(rng() % (top + 1));
        if (round % 5 == 0) counts[(size_t)(rng() % n)] = 0;
        const size_t pair_bytes = round % 2 ? scope::kPairBytesSelection : scope::kPairBytesAllRecords;
        const size_t budget = round % 7 == 0 ? (size_t)1 << 16 : round % 7 == 1 ? (size_t)1 << 24 : escalation::kPassWorkspaceBytes;
        const auto slices = scope::slice_by_pairs(counts, pair_bytes, budget);
        int32_t next = 0;
        for (const auto &s : slices) {
            CHECK(s.first == next && s.second > s.first);              // consecutive, none empty: every query exactly once
            next = s.second;
            uint32_t worst = 0;
            for (int32_t i = s.first; i < s.second; ++i) worst = std::max(worst, counts[(size_t)i]);
            const size_t bytes = (size_t)(s.second - s.first) * scope::slice_cap(worst) * pair_bytes;
            CHECK(bytes <= budget || s.second - s.first == 1);          // within the budget, or one query alone
            // greedy: the next query would not have fitted
            if (s.second < n) {
                const uint32_t w2 = std::max(worst, counts[(size_t)s.second]);
                CHECK((size_t)(s.second + 1 - s.first) * scope::slice_cap(w2) * pair_bytes > budget);
            }
        }
        CHECK(next == n);
    }
    CHECK(scope::slice_by_pairs({}, 40, 1 << 20).empty());
    CHECK(scope::pair_bytes_selection(0) == scope::kPairBytesSelection && scope::pair_bytes_selection(64) == 40);
    CHECK(scope::pair_bytes_selection(16) == 88 && scope::pair_bytes_selection(4) == 280);
    // the largest scope one query may bring fills the tail's grid dimension exactly, and alone stays within the workspace budget
    CHECK(scope::slice_cap(scope::kMaxScopeRows) / 64 == 65535);
    CHECK((size_t)scope::slice_cap(scope::kMaxScopeRows) * scope::pair_bytes_selection(4) <= escalation::kPassWorkspaceBytes);
    CHECK(scope::slice_cap(0) == 64 && scope::slice_cap(64) == 64 && scope::slice_cap(65) == 128);
    CHECK(scope::bitmap_bytes(1) == 16 && scope::bitmap_bytes(128) == 16 && scope::bitmap_bytes(129) == 32);
    CHECK(scope::bitmap_slice(300, 10000000, escalation::kPassWorkspaceBytes) == 300);
    CHECK(scope::bitmap_slice(300, 10000000, (size_t)100 << 20) == 83);          // 1.25 MB per query
    CHECK(scope::bitmap_slice(5, 1 << 30, 1024) == 1);
}

static void test_offsets()
{
    const uint64_t ok[] = {0, 3, 3, 10}, dec[] = {0, 5, 4, 10}, short_end[] = {0, 3, 3, 9}, late[] = {1, 3, 3, 10};
    CHECK(scope::offsets_valid(ok, 3, 10));
    CHECK(!scope::offsets_valid(dec, 3, 10));
    CHECK(!scope::offsets_valid(short_end, 3, 10));
    CHECK(!scope::offsets_valid(late, 3, 10));
    CHECK(scope::offsets_valid(nullptr, 3, 10));
    CHECK(scope::offsets_valid(nullptr, 3, 0));
    CHECK(!scope::offsets_valid(nullptr, 3, -1));
    const uint64_t zero[] = {0, 0};
    CHECK(scope::offsets_valid(zero, 1, 0));
}

// the clip restated bit by bit: walk the bitmap in candidate order and keep a set bit while fewer than `limit` were kept
static std::vector<uint32_t> clip_scalar(const std::vector<uint32_t> &bm, uint64_t limit)
{
    std::vector<uint32_t> out(bm.size(), 0u);
    uint64_t kept = 0;
    for (size_t r = 0; r < bm.size() * 32; ++r)
        if ((bm[r >> 5] >> (r & 31)) & 1u) {
            if (kept < limit) { out[r >> 5] |= 1u << (r & 31); ++kept; }
        }
    return out;
}

static void test_clip()
{
    std::mt19937_64 rng(11);
    for (int round = 0; round < 600; ++round) {
        const size_t words = 1 + rng() % 40;
        std::vector<uint32_t> bm(words);
        const int density = round % 4;                                  // sparse, half, dense, full
        for (auto &w : bm) {
            w = (uint32_t)rng();
            if (density == 0) w &= (uint32_t)rng() & (uint32_t)rng() & (uint32_t)rng();
            if (density == 2) w |= (uint32_t)rng() | (uint32_t)rng();
            if (density == 3) w = 0xFFFFFFFFu;
        }
        if (round % 9 == 0) bm[rng() % words] = 0;
        uint64_t pop = 0;
        for (uint32_t w : bm) pop += (uint64_t)__builtin_popcount(w);
        const uint64_t limits[] = {0, 1, pop ? pop - 1 : 0, pop, pop + 1, pop + 1000, rng() % (pop + 2), ~(uint64_t)0};
        for (uint64_t limit : limits) {
            const std::vector<uint32_t> want = clip_scalar(bm, limit);
            uint64_t before = 0, kept = 0;
            for (size_t i = 0; i < words; ++i) {
                const uint32_t got = scope::clip_word(bm[i], before, limit);
                CHECK(got == want[i]);
                CHECK((got & ~bm[i]) == 0);
                before += (uint64_t)__builtin_popcount(bm[i]);          // the prefix counts the unclipped bits, as the kernel's does
                kept += (uint64_t)__builtin_popcount(got);
            }
            CHECK(kept == std::min(pop, limit));
        }
    }
    CHECK(scope::clip_word(0xFFFFFFFFu, 0, 0) == 0u);
    CHECK(scope::clip_word(0xFFFFFFFFu, 0, 1) == 1u);
    CHECK(scope::clip_word(0xFFFFFFFFu, 0, 32) == 0xFFFFFFFFu);
    CHECK(scope::clip_word(0xF0F0F0F0u, 3, 5) == 0x30u);
    CHECK(scope::clip_word(0x80000001u, 9, 10) == 1u);
    CHECK(scope::clip_word(0u, 0, 10) == 0u);
}

int main()
{
    test_form_choice();
    test_ladder_ends();
    test_slices();
    test_offsets();
    test_clip();
    if (g_failed) { printf("orr_scope_plan_selftest: %d checks failed\n", g_failed); return 1; }
    printf("orr_scope_plan_selftest: ok\n");
    return 0;
}
