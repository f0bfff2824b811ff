// orr_diverse_plan_selftest.cpp -- the rules of a diverse search (orr_diverse_plan.h) on the CPU: the argument order, both greedy
// rules against brute-force restatements on random and planted matrices, the kernel's work split.  No HIP, no GPU;
// tests/test_diverse_cpu.py runs it.  Built with -ffp-contract=off like the library.
#include "../orr_diverse_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

void test_arguments()
{
    using diverse::first_invalid;
    // each case holds exactly one error more than the one behind it
    CHECK(first_invalid(true, 99, 0, 7, kNaN) == 1);
    CHECK(first_invalid(false, 99, 0, 7, kNaN) == 2);
    CHECK(first_invalid(false, 99, 57, 7, kNaN) == 2);
    CHECK(first_invalid(false, 99, -3, 7, kNaN) == 2);
    CHECK(first_invalid(false, 57, 56, 7, kNaN) == 3);
    CHECK(first_invalid(false, 11, 10, 7, kNaN) == 3);
    CHECK(first_invalid(false, 10, 10, 7, kNaN) == 4);
    CHECK(first_invalid(false, 10, 10, -1, kNaN) == 4);
    CHECK(first_invalid(false, 10, 10, 2, kNaN) == 4);
    CHECK(first_invalid(false, 10, 10, diverse::Collapse, kNaN) == 5);
    CHECK(first_invalid(false, 10, 10, diverse::Mmr, kNaN) == 5);
    CHECK(first_invalid(false, 10, 10, diverse::Mmr, 1.0000000000000002) == 6);
    CHECK(first_invalid(false, 10, 10, diverse::Mmr, -4.9e-324) == 6);
    CHECK(first_invalid(false, 10, 10, diverse::Mmr, kInf) == 6);
    CHECK(first_invalid(false, 10, 10, diverse::Mmr, 0.0) == 0);
    CHECK(first_invalid(false, 10, 10, diverse::Mmr, -0.0) == 0);
    CHECK(first_invalid(false, 10, 10, diverse::Mmr, 1.0) == 0);
    CHECK(first_invalid(false, 10, 10, diverse::Collapse, 7.5) == 0);        // any number is a max_cosine
    CHECK(first_invalid(false, 10, 10, diverse::Collapse, -kInf) == 0);
    CHECK(first_invalid(false, 10, 10, diverse::Collapse, kInf) == 0);
    CHECK(first_invalid(false, 0, 1, diverse::Collapse, 0.5) == 0);          // topk 0 takes one
    CHECK(first_invalid(false, -5, 1, diverse::Collapse, 0.5) == 0);
    CHECK(first_invalid(false, 56, 56, diverse::Collapse, 0.5) == 0);
    CHECK(diverse::kMaxPool == 56 && diverse::kPairsPerThread == 7 && diverse::kMaxPairs == 1596);
    CHECK(diverse::mode_valid(0) && diverse::mode_valid(1) && !diverse::mode_valid(2) && !diverse::mode_valid(-1));
    CHECK(diverse::pool_valid(1) && diverse::pool_valid(56) && !diverse::pool_valid(0) && !diverse::pool_valid(57));

    using diverse::first_invalid_pairs;
    CHECK(first_invalid_pairs(true, -1, true, true, 57) == 1);
    CHECK(first_invalid_pairs(false, -1, true, true, 57) == 2);
    CHECK(first_invalid_pairs(false, 3, true, true, 57) == 3);
    CHECK(first_invalid_pairs(false, 3, true, true, 0) == 3);
    CHECK(first_invalid_pairs(false, 3, true, true, 56) == 4);
    CHECK(first_invalid_pairs(false, 3, false, true, 56) == 5);
    CHECK(first_invalid_pairs(false, 3, false, false, 56) == 0);
    CHECK(first_invalid_pairs(false, 0, false, false, 1) == 0);

    using diverse::needs_dots;
    CHECK(!needs_dots(diverse::Collapse, 0.5, 1, 128) && !needs_dots(diverse::Collapse, 0.5, 0, 128) && !needs_dots(diverse::Mmr, 0.5, 1, 128));
    CHECK(!needs_dots(diverse::Collapse, 0.5, 9, 0) && !needs_dots(diverse::Mmr, 0.5, 9, 0));
    CHECK(!needs_dots(diverse::Collapse, kInf, 9, 128) && needs_dots(diverse::Collapse, -kInf, 9, 128) && needs_dots(diverse::Collapse, 1e308, 2, 1));
    CHECK(!needs_dots(diverse::Mmr, 1.0, 9, 128) && needs_dots(diverse::Mmr, 0.9999999999999999, 9, 128) && needs_dots(diverse::Mmr, 0.0, 2, 1));
}

void test_small_rules()
{
    using namespace diverse;
    CHECK(!collapse_keeps(0.5, 0.5) && collapse_keeps(0.49999999999999994, 0.5) && !collapse_keeps(0.6, 0.5));
    CHECK(collapse_keeps(kNaN, 0.5) && collapse_keeps(kNaN, -kInf) && collapse_keeps(kInf, kNaN));   // a NaN never drops
    CHECK(!collapse_keeps(-1.0, -kInf) && !collapse_keeps(kInf, kInf) && collapse_keeps(1e308, kInf) && !collapse_keeps(-kInf, -kInf));
    CHECK(mmr_fold(-kInf, kNaN) == -kInf && mmr_fold(-kInf, -2.0) == -2.0 && mmr_fold(0.3, 0.2) == 0.3 && mmr_fold(0.3, kInf) == kInf);
    CHECK(mmr_fold(-kInf, -kInf) == -kInf && mmr_penalty_cosine(-kInf) == 0.0 && mmr_penalty_cosine(-0.25) == -0.25);
    CHECK(mmr_value(1.0, 0.75, kInf) == 0.75 && mmr_value(1.0, 0.75, kNaN) == 0.75 && mmr_value(1.0, -0.0, 5.0) == 0.0);
    CHECK(mmr_value(0.0, 123.0, 0.5) == -0.5 && mmr_value(0.0, kInf, 0.5) != mmr_value(0.0, kInf, 0.5));       // 0 * inf is NaN
    CHECK(mmr_value(0.3, 0.9, 0.8) == (0.3 * 0.9) - ((1.0 - 0.3) * 0.8));
    CHECK(compare_double(kNaN, -kInf) < 0 && compare_double(kNaN, kNaN) == 0 && compare_double(1.0, kNaN) > 0 && compare_double(0.0, -0.0) == 0);
    CHECK(take_of(0) == 1 && take_of(-9) == 1 && take_of(1) == 1 && take_of(10) == 10);
}

// ---- brute-force restatements: no incremental state, every value from its definition ---------------------------------------
std::vector<int32_t> brute_collapse(int32_t n, int32_t take, double t, const std::vector<double> &c)
{
    std::vector<int32_t> kept;
    for (int32_t r = 0; r < n; ++r) {
        if ((int32_t)kept.size() == take) break;
        bool dropped = false;
        for (int32_t k : kept)
            if (c[(size_t)r * n + k] >= t) dropped = true;
        if (!dropped) kept.push_back(r);
    }
    return kept;
}

std::vector<int32_t> brute_mmr(int32_t n, int32_t take, double lambda, const std::vector<double> &score, const std::vector<double> &c)
{
    std::vector<int32_t> kept;
    if (n == 0) return kept;
    kept.push_back(0);
    while ((int32_t)kept.size() < take && (int32_t)kept.size() < n) {
        int32_t best = -1;
        double best_v = 0.0;
        for (int32_t r = n - 1; r >= 0; --r) {                 // downwards, ties (>=) to the lower rank: the other way round
            if (std::find(kept.begin(), kept.end(), r) != kept.end()) continue;
            double m = -kInf;
            for (int32_t k : kept) { const double x = c[(size_t)r * n + k]; if (x > m) m = x; }
            if (m == -kInf) m = 0.0;
            volatile double gain = lambda * score[(size_t)r];
            volatile double w = 1.0 - lambda;
            volatile double pen = w == 0.0 ? 0.0 : w * m;
            const double v = gain - pen;
            if (best < 0 || diverse::compare_double(v, best_v) >= 0) { best = r; best_v = v; }
        }
        kept.push_back(best);
    }
    return kept;
}

struct Case { int32_t n; std::vector<double> score, c; };

Case random_case(std::mt19937_64 &rng, int32_t n, int planted)
{
    Case k;
    k.n = n;
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    k.score.resize((size_t)n);
    for (double &s : k.score) s = u(rng);
    std::sort(k.score.begin(), k.score.end(), [](double a, double b) { return a > b; });
    k.c.assign((size_t)n * n, 0.0);
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = i; j < n; ++j) {
            double v = i == j ? 1.0 : u(rng);
            if (planted >= 1 && i != j) v = std::round(v * 4.0) / 4.0;                       // many equal cosines: ties, borders
            if (planted >= 2 && i != j) {
                const uint64_t z = rng() % 16;
                if (z == 0) v = kNaN; else if (z == 1) v = kInf; else if (z == 2) v = -kInf;
            }
            k.c[(size_t)i * n + j] = k.c[(size_t)j * n + i] = v;
        }
    if (planted >= 1) for (double &s : k.score) s = std::round(s * 3.0) / 3.0;              // equal scores
    if (planted >= 3) {
        for (double &s : k.score) { const uint64_t z = rng() % 12; if (z == 0) s = kNaN; else if (z == 1) s = kInf; else if (z == 2) s = -kInf; }
        if (n > 2) k.c[(size_t)1 * n + 1] = kNaN;                                            // the diagonal is never read
    }
    return k;
}

void test_greedy_rules()
{
    std::mt19937_64 rng(20240607);
    const double thresholds[] = {0.95, 0.5, 0.25, 0.0, -0.25, -1.0, 1.0, kInf, -kInf};
    const double lambdas[] = {0.0, 0.3, 0.5, 0.7, 1.0, 0.9999999999999999, 4.9e-324};
    const int32_t sizes[] = {1, 2, 3, 7, 24, 55, 56};
    int64_t cases = 0, shorter = 0, reordered = 0;
    for (int planted = 0; planted <= 3; ++planted)
        for (int32_t n : sizes)
            for (int rep = 0; rep < 6; ++rep) {
                const Case k = random_case(rng, n, planted);
                auto cosine = [&](int32_t i, int32_t j) { return k.c[(size_t)i * n + j]; };
                const int32_t takes[] = {1, 4, 10, n};
                for (int32_t take : takes) {
                    if (take > n) continue;
                    std::vector<int32_t> picks((size_t)take, -7);
                    for (double t : thresholds) {
                        std::fill(picks.begin(), picks.end(), -7);
                        const int32_t got = diverse::select_collapse(n, take, t, cosine, picks.data());
                        const std::vector<int32_t> want = brute_collapse(n, take, t, k.c);
                        CHECK(got == (int32_t)want.size() && std::equal(want.begin(), want.end(), picks.begin()));
                        for (int32_t i = got; i < take; ++i) CHECK(picks[(size_t)i] == -7);
                        if (t == kInf && planted < 2) {                                                      // the plain order
                            CHECK(got == take);
                            for (int32_t i = 0; i < got; ++i) CHECK(picks[(size_t)i] == i);
                        }
                        if (t == -kInf && planted < 2) CHECK(got == 1);                                      // everything is a duplicate
                        shorter += got < take;
                        ++cases;
                    }
                    for (double l : lambdas) {
                        std::fill(picks.begin(), picks.end(), -7);
                        const int32_t got = diverse::select_mmr(n, take, l, k.score.data(), cosine, picks.data());
                        const std::vector<int32_t> want = brute_mmr(n, take, l, k.score, k.c);
                        CHECK(got == take && got == (int32_t)want.size() && std::equal(want.begin(), want.end(), picks.begin()));
                        CHECK(picks[0] == 0);
                        std::vector<int32_t> sorted(picks.begin(), picks.begin() + got);
                        std::sort(sorted.begin(), sorted.end());
                        CHECK(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end());             // no member twice
                        if (l == 1.0 && planted < 3) for (int32_t i = 0; i < got; ++i) CHECK(picks[(size_t)i] == i);
                        for (int32_t i = 0; i < got; ++i) reordered += picks[(size_t)i] != i;
                        ++cases;
                    }
                }
            }
    CHECK(shorter > 0 && reordered > 0);
    // lambda = 1 with NaN scores: compare_double's order, the lower rank on a tie -- the plain order of a list the search sorted
    {
        const double score[] = {kInf, 2.0, 2.0, -kInf, kNaN, kNaN};
        int32_t picks[6];
        auto cosine = [](int32_t, int32_t) { return kNaN; };
        CHECK(diverse::select_mmr(6, 6, 1.0, score, cosine, picks) == 6);
        for (int32_t i = 0; i < 6; ++i) CHECK(picks[i] == i);
    }
    // a planted tie: members 1 and 2 have the same value, the lower rank goes first; member 3 wins over both once 1 is in
    {
        const double score[] = {1.0, 0.5, 0.5, 0.5};
        const double c[16] = {1, 0.5, 0.5, 0.5,   0.5, 1, 1.0, 0.0,   0.5, 1.0, 1, 0.0,   0.5, 0.0, 0.0, 1};
        int32_t picks[4];
        auto cosine = [&](int32_t i, int32_t j) { return c[i * 4 + j]; };
        CHECK(diverse::select_mmr(4, 4, 0.5, score, cosine, picks) == 4);
        CHECK(picks[0] == 0 && picks[1] == 1 && picks[2] == 3 && picks[3] == 2);
        CHECK(diverse::select_collapse(4, 4, 1.0, cosine, picks) == 3 && picks[0] == 0 && picks[1] == 1 && picks[2] == 3);
    }
    printf("greedy cases checked: %lld (collapses shorter than take: %lld, MMR picks out of rank order: %lld)\n", (long long)cases,
           (long long)shorter, (long long)reordered);
}

void test_work_split()
{
    using namespace diverse;
    for (int32_t cnt = 0; cnt <= kMaxPool; ++cnt) {
        const int32_t np = pair_count(cnt);
        CHECK(np <= kPairThreads * kPairsPerThread);
        std::vector<int32_t> seen((size_t)cnt * cnt, 0);
        for (int32_t t = 0; t < kPairThreads; ++t)
            for (int32_t s = 0; s < kPairsPerThread; ++s) {
                const int32_t p = owned_pair(t, s);
                if (p >= np) continue;
                int32_t i = -1, j = -1;
                pair_of(p, cnt, &i, &j);
                CHECK(0 <= i && i <= j && j < cnt);
                if (0 <= i && i <= j && j < cnt) seen[(size_t)i * cnt + j] += 1;
            }
        for (int32_t i = 0; i < cnt; ++i)
            for (int32_t j = 0; j < cnt; ++j) CHECK(seen[(size_t)i * cnt + j] == (i <= j ? 1 : 0));
        // every pair number below np is some thread's
        std::vector<int32_t> owner((size_t)np, 0);
        for (int32_t t = 0; t < kPairThreads; ++t)
            for (int32_t s = 0; s < kPairsPerThread; ++s)
                if (owned_pair(t, s) < np) owner[(size_t)owned_pair(t, s)] += 1;
        for (int32_t p = 0; p < np; ++p) CHECK(owner[(size_t)p] == 1);
    }
    CHECK(mat_index(56, 3, 5) == 3 * 56 + 5 && mat_index(7, 0, 0) == 0);
}

}  // namespace

int main()
{
    test_arguments();
    test_small_rules();
    test_greedy_rules();
    test_work_split();
    if (g_fail) { fprintf(stderr, "orr_diverse_plan_selftest: %d check(s) failed\n", g_fail); return 1; }
    printf("orr_diverse_plan_selftest: ok\n");
    return 0;
}
