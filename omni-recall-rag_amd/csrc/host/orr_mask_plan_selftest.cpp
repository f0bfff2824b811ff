// orr_mask_plan_selftest -- the rules of orr_mask_plan.h on the CPU (no HIP, no GPU): the sample size and its clamps,
// eligibility, the cost rule, the ladder and its bound, the parts of the list path against a scalar restatement of a bitmap,
// mask_survivors' per-entry decision, and the workspace slices.
// Exit status 0 and a last line "orr_mask_plan_selftest: ok" when everything holds; tests/test_mask_plan_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../orr_mask_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static void test_sentinel()
{
    // finite in fp64 and in fp32, and below every floor a finite query can have (scores lie above -2)
    CHECK(mask::kMaskedRecency < -1e6 && mask::kMaskedRecency > -3.0e38);
    const float f = (float)mask::kMaskedRecency;
    CHECK(f == f && f > -3.0e38f && f < -1e29f);
    CHECK(0.2 + mask::kMaskedRecency + 2.0 < -2.0);                 // the best a masked row's bound can be: keyword credit + bounds
}

static void test_sample()
{
    for (int32_t k : {0, 1, 10, 40, 64})
        for (int64_t took : {1ll, 100ll, 5000ll, 20000ll, 100000ll, 1000000ll, 10000000ll, 1ll << 33}) {
            const int64_t m = mask::sample_rows(k, took);
            CHECK(m % 64 == 0);                                       // whole selection lists
            CHECK(m >= mask::kMinSampleRows && m >= 4 * (int64_t)std::max(1, k));
            CHECK(m <= mask::kMaxSampleRows);
            CHECK(mask::sample_rows(k, took * 2) >= m);               // monotone in the scope
        }
    // between the clamps it is sqrt(k took) in whole lists
    CHECK(mask::sample_rows(10, 100000) == 1024);                    // sqrt(1e6) = 1000
    CHECK(mask::sample_rows(10, 20000) == 448);                      // sqrt(2e5) = 447.2
    CHECK(mask::sample_rows(40, 1000000) == 6336);                   // sqrt(4e7) = 6324.6
    CHECK(mask::sample_rows(10, 1000) == 256);                       // lower clamp
    CHECK(mask::sample_rows(64, 1ll << 40) == 65536);                // upper clamp
}

static void test_eligibility_and_cost()
{
    const int64_t n = mask::kMinScreenRows;
    CHECK(n == 196608);
    CHECK(mask::eligible(true, 128, 10, 64, n, 1, 20000));
    CHECK(!mask::eligible(false, 128, 10, 64, n, 1, 20000));        // no cosine part
    CHECK(!mask::eligible(true, 100, 10, 64, n, 1, 20000));         // dim % 64
    CHECK(!mask::eligible(true, 128, 65, 64, n, 1, 20000));         // topk beyond a selection list
    CHECK(mask::eligible(true, 128, 0, 64, n, 1, 20000));           // topk 0 asks for one
    CHECK(!mask::eligible(true, 128, 10, 64, n - 1, 1, 20000));     // too few rows in front of the scope's last
    CHECK(!mask::eligible(true, 128, 10, 64, n, 0, 20000));         // two_stage off
    CHECK(mask::eligible(true, 128, 10, 64, n, 2, 20000));
    CHECK(!mask::eligible(true, 128, 10, 64, n, 1, 256));           // a scope no larger than its sample
    CHECK(mask::eligible(true, 128, 10, 64, n, 1, 257));
    // max(4 B, 128) took >= n_clip: the byte model from 32 queries on, the measured floor of 128 below
    CHECK(mask::screen_pays(256, 1000, 1000000) && mask::screen_pays(256, 977, 1000000) && !mask::screen_pays(256, 976, 1000000));
    CHECK(mask::screen_pays(1, 7813, 1000000) && !mask::screen_pays(1, 7812, 1000000));
    CHECK(mask::screen_pays(8, 7813, 1000000) && !mask::screen_pays(8, 7812, 1000000));
    CHECK(mask::screen_pays(32, 7813, 1000000) && !mask::screen_pays(32, 7812, 1000000));
    CHECK(mask::screen_pays(33, 7576, 1000000) && !mask::screen_pays(33, 7575, 1000000));
    // what was measured at 1M x 3072: the masked call wins at 30,000 rows for 1 and 8 queries and loses at 3,000; at 256 it wins from 3,000 on
    CHECK(!mask::screen_pays(1, 3000, 1000000) && mask::screen_pays(1, 30000, 1000000));
    CHECK(!mask::screen_pays(8, 3000, 1000000) && mask::screen_pays(8, 30000, 1000000));
    CHECK(mask::screen_pays(256, 3000, 1000000));
    CHECK(mask::screen_pays(1 << 30, (int64_t)1 << 40, (int64_t)1 << 62));      // no overflow in the product
    using mask::Path;
    CHECK(mask::choose(0, true, 256, 1000, 1000000) == Path::Screen);
    CHECK(mask::choose(0, true, 1, 1000, 1000000) == Path::List);
    CHECK(mask::choose(1, true, 1, 1000, 1000000) == Path::Screen);
    CHECK(mask::choose(1, false, 256, 1000, 1000000) == Path::List);
    CHECK(mask::choose(2, true, 256, 500000, 1000000) == Path::List);
}

static void test_ladder()
{
    using mask::Step;
    // overflow as the only reason, buffers that can hold it: grow once
    mask::Next n = mask::next_step(true, false, 8192, 20000, 200000, 8, 32, 64);
    CHECK(n.step == Step::GrowBuffers && n.new_cap == 32768 && n.kprime == 32);
    // ... not twice
    n = mask::next_step(true, true, 32768, 40000, 200000, 8, 32, 64);
    CHECK(n.step == Step::ListParts);
    // too many survivors to buffer
    n = mask::next_step(true, false, 8192, 150000, 200000, 8, 32, 64);
    CHECK(n.step == Step::ListParts);
    // a tie at the cut with a small k'
    n = mask::next_step(false, false, 8192, 0, 200000, 8, 4, 64);
    CHECK(n.step == Step::WiderK && n.kprime == 16);
    n = mask::next_step(false, false, 8192, 0, 200000, 8, 16, 64);
    CHECK(n.step == Step::WiderK && n.kprime == 64);
    n = mask::next_step(false, false, 8192, 0, 200000, 8, 32, 64);
    CHECK(n.step == Step::ListParts);
    // every walk ends in ListParts within kMaxScreenRepeats repeats, whatever the pass reports
    std::mt19937 rng(7);
    for (int trial = 0; trial < 2000; ++trial) {
        int64_t kprime = 1 + (int64_t)(rng() % 64);
        bool grown = false;
        uint32_t cap = 8192;
        int repeats = 0;
        for (;;) {
            const bool only_overflow = rng() % 2;
            const uint32_t worst = cap + 1 + rng() % (1u << 20);
            n = mask::next_step(only_overflow, grown, cap, worst, 1 << 22, 1 + rng() % 256, kprime, 64);
            if (n.step == Step::ListParts) break;
            if (n.step == Step::GrowBuffers) { CHECK(!grown && n.new_cap > cap && n.new_cap >= worst); grown = true; cap = n.new_cap; }
            if (n.step == Step::WiderK) { CHECK(n.kprime == kprime * 4 && n.kprime <= 64); }
            kprime = n.kprime;
            ++repeats;
            CHECK(repeats <= mask::kMaxScreenRepeats);
            if (repeats > mask::kMaxScreenRepeats) break;
        }
    }
}

static void test_parts()
{
    CHECK(mask::kDefaultPartRows == 4194240);
    CHECK(mask::part_rows_valid(1) && mask::part_rows_valid(4194240) && !mask::part_rows_valid(0) && !mask::part_rows_valid(4194241));
    CHECK(mask::part_count(0, 5000) == 0 && mask::part_count(1, 5000) == 1 && mask::part_count(5000, 5000) == 1 && mask::part_count(5001, 5000) == 2);
    CHECK(mask::part_count(10000000, mask::kDefaultPartRows) == 3);  // beyond the scoped call's limit: three parts
    // the parts tile [0, took) in order
    for (int64_t took : {1ll, 4999ll, 5000ll, 5001ll, 12345ll, 20000ll})
        for (int64_t rows : {1ll, 7ll, 5000ll, 100000ll}) {
            const int64_t P = mask::part_count(took, rows);
            int64_t at = 0;
            for (int64_t j = 0; j < P; ++j) {
                const auto r = mask::part_range(j, took, rows);
                CHECK(r.first == at && r.second > r.first && r.second - r.first <= rows);
                CHECK(mask::part_limit(took, r.first) == took - r.first);      // what is left of the limit for this part and those behind
                at = r.second;
            }
            CHECK(at == took);
        }
    CHECK(mask::part_limit(12000, 15000) == 0);
    // part_word against a scalar restatement over a random bitmap: every set bit of rank [first, last), nothing else
    std::mt19937 rng(11);
    for (int trial = 0; trial < 200; ++trial) {
        std::vector<uint32_t> bm(64);
        for (auto &w : bm) w = (trial % 3 == 0) ? rng() & rng() : (trial % 3 == 1) ? rng() | rng() : rng();
        uint64_t total = 0;
        for (uint32_t w : bm) total += (uint64_t)__builtin_popcount(w);
        const uint64_t first = rng() % (total + 2), last = first + rng() % (total + 2 - first + 1);
        uint64_t before = 0, rank = 0;
        for (size_t i = 0; i < bm.size(); ++i) {
            uint32_t want = 0;
            for (int b = 0; b < 32; ++b)
                if ((bm[i] >> b) & 1u) { if (rank >= first && rank < last) want |= 1u << b; ++rank; }
            CHECK(mask::part_word(bm[i], before, first, last) == want);
            before += (uint64_t)__builtin_popcount(bm[i]);
        }
    }
    // merges stay within the budget, with at least one query
    CHECK(mask::merge_group(40, 4, 5000, mask::kMergeBudgetBytes) == 40);
    CHECK(mask::merge_group(256, 3, 4194240, mask::kMergeBudgetBytes) == 1);
    const int32_t g = mask::merge_group(256, 4, 100000, mask::kMergeBudgetBytes);
    CHECK(g >= 1 && (size_t)g * 4 * 100001 * mask::kRecordBytes <= mask::kMergeBudgetBytes);
}

static void test_survivor_decision()
{
    std::vector<uint32_t> bm(8, 0u);
    bm[0] = 0x5u; bm[3] = 0x80000000u; bm[7] = 1u;
    CHECK(mask::survivor_in_scope(bm.data(), 0, 256) && !mask::survivor_in_scope(bm.data(), 1, 256) && mask::survivor_in_scope(bm.data(), 2, 256));
    CHECK(mask::survivor_in_scope(bm.data(), 127, 256) && !mask::survivor_in_scope(bm.data(), 126, 256));
    CHECK(mask::survivor_in_scope(bm.data(), 224, 256));
    CHECK(!mask::survivor_in_scope(bm.data(), 224, 224));            // a set bit behind the clip does not take part
    CHECK(mask::survivor_in_scope(bm.data(), 127, 128) && !mask::survivor_in_scope(bm.data(), 127, 127));
    CHECK(!mask::survivor_in_scope(bm.data(), 0xFFFFFFFFu, 256));    // an entry past the clip is never looked up
}

static void test_workspace()
{
    for (int32_t B : {1, 8, 256, 4096, 100000})
        for (int64_t sample : {256ll, 1024ll, 65536ll}) {
            const int32_t per = mask::screen_slice(B, sample);
            CHECK(per >= 1 && per <= B);
            const size_t per_query = mask::kPairBytes * (size_t)std::max<int64_t>(sample, mask::kMinPassCap);
            CHECK(per == 1 || (size_t)per * per_query <= escalation::kPassWorkspaceBytes);
        }
    CHECK(mask::screen_slice(256, 1024) == 256);                     // the bench's batches go in one piece
}

int main()
{
    test_sentinel();
    test_sample();
    test_eligibility_and_cost();
    test_ladder();
    test_parts();
    test_survivor_decision();
    test_workspace();
    if (g_failed) { printf("orr_mask_plan_selftest: %d checks FAILED\n", g_failed); return 1; }
    printf("orr_mask_plan_selftest: ok\n");
    return 0;
}
