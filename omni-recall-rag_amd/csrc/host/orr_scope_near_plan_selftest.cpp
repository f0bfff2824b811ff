// orr_scope_near_plan_selftest -- the rules of orr_scope_near_plan.h on the CPU (no HIP, no GPU): the cosine and its guards, the
// fold and the row rule for 1, 2 and 8 probes against a restatement, in_band on both sides of the border and at +-0,
// +-infinity and NaN, the host's decision of a pending row, the tail mask at every kind of last word, the validity rules in
// their order, the foreign-dim rule and the band list's growth.
// Exit status 0 and a last line "orr_scope_near_plan_selftest: ok" when everything holds; tests/test_scope_near_cpu.py runs it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../orr_scope_near_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kBand = 0x1p-40;               // the band's absolute width for |c| <= 2

static int64_t words_for(int64_t rows) { return ((rows + 31) / 32 + 3) / 4 * 4; }

static void test_cosine()
{
    // RecallSearchService.cs:84-87, written out once more
    CHECK(scope_near::cosine_of(3.0, 0.0, 4.0) == 0.0 && scope_near::cosine_of(3.0, 4.0, 0.0) == 0.0);
    CHECK(scope_near::cosine_of(3.0, -1.0, 4.0) == 0.0 && scope_near::cosine_of(kNaN, 0.0, 4.0) == 0.0);
    CHECK(scope_near::cosine_of(6.0, 4.0, 9.0) == 6.0 / (std::sqrt(4.0) * std::sqrt(9.0)));
    CHECK(scope_near::cosine_of(6.0, 4.0, 9.0) == 1.0);
    CHECK(std::isnan(scope_near::cosine_of(1.0, kNaN, 4.0)));            // NaN <= 0 is false: the division runs
    CHECK(std::isnan(scope_near::cosine_of(kInf, kInf, 4.0)));           // infinity / infinity
    CHECK(scope_near::cosine_of(1.0, kInf, 4.0) == 0.0);                 // a row whose squares overflow: finite / infinity
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> u(1e-3, 1e3);
    for (int i = 0; i < 1000; ++i) {
        const double d = u(rng) - 500.0, a = u(rng), b = u(rng);
        CHECK(scope_near::cosine_of(d, a, b) == d / (std::sqrt(a) * std::sqrt(b)));
    }
    // verdict is C#'s >= on doubles
    CHECK(scope_near::verdict(0.5, 0.5) && scope_near::verdict(0.5, -kInf) && !scope_near::verdict(0.5, kInf));
    CHECK(!scope_near::verdict(kNaN, -kInf) && !scope_near::verdict(kNaN, 0.0) && scope_near::verdict(-0.0, 0.0) && scope_near::verdict(0.0, -0.0));
}

static void test_in_band()
{
    for (double t : {-1.0, -0.25, 0.0, -0.0, 0.05, 0.2, 0.999, 1.0, 2.0}) {
        CHECK(scope_near::in_band(t, t));
        CHECK(scope_near::in_band(t + kBand / 2, t) && scope_near::in_band(t - kBand / 2, t));
        CHECK(scope_near::in_band(std::nextafter(t, 9.0), t) && scope_near::in_band(std::nextafter(t, -9.0), t));
        CHECK(!scope_near::in_band(t + 4 * kBand, t) && !scope_near::in_band(t - 4 * kBand, t));
        CHECK(!scope_near::in_band(t + 0.01, t) && !scope_near::in_band(t - 0.01, t));
    }
    // the border itself: exactly the width is still in the band, the next double beyond it is not (t = 0: the difference is exact)
    CHECK(scope_near::in_band(kBand, 0.0) && !scope_near::in_band(std::nextafter(kBand, 1.0), 0.0));
    CHECK(scope_near::in_band(-kBand, 0.0) && !scope_near::in_band(std::nextafter(-kBand, -1.0), 0.0));
    CHECK(scope_near::in_band(0.0, -0.0) && scope_near::in_band(-0.0, 0.0));
    // a band at least the documented worst case of the device's arithmetic for |c| <= 2 (40 * 2^-53 * 2 < 2^-46), with room
    CHECK(scope_near::band_width(0.0) == kBand && scope_near::band_width(-2.0) == kBand && scope_near::band_width(1.0) >= 64 * 0x1p-46);
    CHECK(scope_near::band_width(8.0) == 4 * kBand && scope_near::band_width(-8.0) == 4 * kBand);   // relative above 2
    // +-infinity as the threshold: never in the band, whatever finite c is
    for (double c : {-1.0, 0.0, 1.0, 1e300}) CHECK(!scope_near::in_band(c, kInf) && !scope_near::in_band(c, -kInf));
    // a cosine that is not finite always is: the host decides it
    for (double t : {-kInf, -1.0, 0.0, 1.0, kInf})
        CHECK(scope_near::in_band(kNaN, t) && scope_near::in_band(kInf, t) && scope_near::in_band(-kInf, t));
}

// a row's state, a pair at a time: undecided pairs may fall either way; the row is settled iff both ways give the same bit
static int32_t state_by_cases(const std::vector<double> &c, double t, int32_t mode)
{
    if (c.empty()) return scope_near::Out;
    bool any_band = false;
    int res[2];
    for (int way = 0; way < 2; ++way) {
        size_t held = 0;
        for (double x : c) {
            const bool band = !std::isfinite(x) || !(std::fabs(x - t) > scope_near::band_width(x));
            any_band |= band;
            held += band ? (size_t)way : (size_t)(x >= t);
        }
        res[way] = mode == scope_near::All ? held == c.size() : held > 0;
    }
    if (res[0] == res[1]) return res[0] ? scope_near::In : scope_near::Out;
    (void)any_band;
    return scope_near::Pending;
}

static void test_fold_and_rows()
{
    CHECK(scope_near::fold_identity(scope_near::All) && !scope_near::fold_identity(scope_near::Any));
    for (int32_t mode : {(int32_t)scope_near::All, (int32_t)scope_near::Any})
        for (int a = 0; a < 2; ++a) {
            for (int v = 0; v < 2; ++v) CHECK(scope_near::fold_verdict(a, v, mode) == (mode == scope_near::All ? (a && v) : (a || v)));
            CHECK(scope_near::fold_settled(a, mode) == (mode == scope_near::All ? !a : (bool)a));
        }
    std::mt19937 rng(11);
    const double t = 0.25;
    // a pair is: clearly in, clearly out, in the band above, in the band below, NaN
    const double kinds[5] = {0.9, -0.3, t + kBand / 4, t - kBand / 4, kNaN};
    for (int32_t n : {1, 2, 8})
        for (int rep = 0; rep < 4000; ++rep) {
            std::vector<double> c((size_t)n);
            for (auto &x : c) x = kinds[rng() % (rep % 3 == 0 ? 2 : 5)];
            if (rep % 7 == 5 && n > 1) c[1] = c[0];                              // the same probe twice
            for (int32_t mode : {(int32_t)scope_near::All, (int32_t)scope_near::Any}) {
                const int32_t st = scope_near::row_state(c.data(), n, t, mode);
                CHECK(st == state_by_cases(c, t, mode));
                // the fold of the certain pairs alone, by the inlines
                bool acc = scope_near::fold_identity(mode), band = false;
                for (double x : c) {
                    if (scope_near::in_band(x, t)) band = true;
                    else acc = scope_near::fold_verdict(acc, scope_near::verdict(x, t), mode);
                }
                if (!band) CHECK(st == (acc ? scope_near::In : scope_near::Out));
                if (st == scope_near::Pending) {
                    // the host's fold of the band pairs alone, from the identity, is the fold of ALL pairs with the band decided exactly
                    std::vector<double> bc;
                    size_t held = 0;
                    for (double x : c) {
                        if (scope_near::in_band(x, t)) bc.push_back(x);
                        held += x >= t;
                    }
                    const bool want = mode == scope_near::All ? held == c.size() : held > 0;
                    CHECK(scope_near::pending_row_in(bc.data(), (int32_t)bc.size(), t, mode) == want);
                }
            }
        }
    // no probes: out in both modes; duplicates change nothing
    CHECK(scope_near::row_state(nullptr, 0, 0.0, scope_near::All) == scope_near::Out);
    CHECK(scope_near::row_state(nullptr, 0, -kInf, scope_near::Any) == scope_near::Out);
    const double two[2] = {0.9, 0.9}, mixed[2] = {0.9, -0.3}, edge[2] = {0.9, t};
    CHECK(scope_near::row_state(two, 2, t, scope_near::All) == scope_near::In && scope_near::row_state(two, 1, t, scope_near::All) == scope_near::In);
    CHECK(scope_near::row_state(mixed, 2, t, scope_near::All) == scope_near::Out && scope_near::row_state(mixed, 2, t, scope_near::Any) == scope_near::In);
    CHECK(scope_near::row_state(edge, 2, t, scope_near::All) == scope_near::Pending);      // the band pair can still empty ALL
    CHECK(scope_near::row_state(edge, 2, t, scope_near::Any) == scope_near::In);           // ... but ANY is settled already
    // +-infinity: everything certain
    const double some[3] = {-1.0, 0.0, 1.0};
    CHECK(scope_near::row_state(some, 3, -kInf, scope_near::All) == scope_near::In && scope_near::row_state(some, 3, kInf, scope_near::Any) == scope_near::Out);
    const double with_nan[2] = {kNaN, 1.0};
    CHECK(scope_near::row_state(with_nan, 2, -kInf, scope_near::All) == scope_near::Pending);
    CHECK(!scope_near::pending_row_in(with_nan, 1, -kInf, scope_near::All));                // NaN is never >=
}

static void test_tail_mask()
{
    for (int64_t n_rows : {1ll, 31ll, 32ll, 33ll, 63ll, 64ll, 65ll, 127ll, 128ll, 129ll, 4099ll, 70001ll, 200000ll, 196608ll, 1000001ll}) {
        const int64_t words = words_for(n_rows);
        CHECK(words % 4 == 0 && words * 32 >= n_rows);
        for (int64_t w = 0; w < words; ++w) {
            uint32_t want = 0;
            for (int b = 0; b < 32; ++b)
                if (w * 32 + b < n_rows) want |= 1u << b;
            if (scope_near::tail_mask(w, n_rows) != want) { CHECK(!"tail_mask differs from the row-by-row mask"); break; }
        }
        const int64_t last = (n_rows - 1) / 32;
        const int rem = (int)(n_rows % 32);
        CHECK(scope_near::tail_mask(last, n_rows) == (rem == 0 ? 0xFFFFFFFFu : (1u << rem) - 1u));
        for (int64_t w = last + 1; w < words; ++w) CHECK(scope_near::tail_mask(w, n_rows) == 0u);
        if (last > 0) CHECK(scope_near::tail_mask(last - 1, n_rows) == 0xFFFFFFFFu);
    }
    CHECK(scope_near::tail_mask(0, 0) == 0u && scope_near::tail_mask(3, 0) == 0u);
}

static void test_arguments()
{
    CHECK(scope_near::All == 0 && scope_near::Any == 1 && scope_near::kMaxProbes == 8);
    CHECK(scope_near::mode_valid(0) && scope_near::mode_valid(1) && !scope_near::mode_valid(-1) && !scope_near::mode_valid(2));
    CHECK(scope_near::probes_valid(0) && scope_near::probes_valid(8) && !scope_near::probes_valid(-1) && !scope_near::probes_valid(9));
    // each case breaks the named rule AND every rule behind it: the first one is reported
    CHECK(scope_near::first_invalid(true, 9, -1, true, 2, kNaN) == 1);
    CHECK(scope_near::first_invalid(false, 9, -1, true, 2, kNaN) == 2 && scope_near::first_invalid(false, -1, -1, true, 2, kNaN) == 2);
    CHECK(scope_near::first_invalid(false, 8, -1, true, 2, kNaN) == 3);
    CHECK(scope_near::first_invalid(false, 8, 4, true, 2, kNaN) == 4);
    CHECK(scope_near::first_invalid(false, 8, 4, false, 2, kNaN) == 5 && scope_near::first_invalid(false, 8, 4, false, -1, kNaN) == 5);
    CHECK(scope_near::first_invalid(false, 8, 4, false, 1, kNaN) == 6);
    CHECK(scope_near::first_invalid(false, 8, 4, false, 1, 0.5) == 0);
    // NULL probes are fine without probes or without a dimension; the infinities are thresholds like any other
    CHECK(scope_near::first_invalid(false, 0, 4, true, 0, 0.5) == 0 && scope_near::first_invalid(false, 3, 0, true, 0, 0.5) == 0);
    CHECK(scope_near::first_invalid(false, 1, 4, false, 0, kInf) == 0 && scope_near::first_invalid(false, 1, 4, false, 0, -kInf) == 0);
    // a foreign dim: all rows or none
    CHECK(scope_near::foreign_dim(0, 128) && scope_near::foreign_dim(64, 128) && scope_near::foreign_dim(0, 0) && scope_near::foreign_dim(4, 0));
    CHECK(!scope_near::foreign_dim(128, 128));
    CHECK(scope_near::all_rows_at_zero(0.0) && scope_near::all_rows_at_zero(-0.0) && scope_near::all_rows_at_zero(-1.0) && scope_near::all_rows_at_zero(-kInf));
    CHECK(!scope_near::all_rows_at_zero(1e-300) && !scope_near::all_rows_at_zero(kInf));
    for (double t : {-1.0, 0.0, 1e-9, 1.0}) CHECK(scope_near::all_rows_at_zero(t) == scope_near::verdict(scope_near::cosine_of(7.0, 0.0, 0.0), t));
}

static void test_growth()
{
    CHECK(scope_near::band_cap_valid(1) && scope_near::band_cap_valid(scope_near::kDefaultBandCap) && scope_near::band_cap_valid(scope_near::kMaxBandCap));
    CHECK(!scope_near::band_cap_valid(0) && !scope_near::band_cap_valid(-5) && !scope_near::band_cap_valid(scope_near::kMaxBandCap + 1));
    for (int64_t count : {17ll, 5000ll, 65537ll, 40000000ll}) {
        const int64_t cap = scope_near::grown_cap(count);
        CHECK(cap >= count && scope_near::band_cap_valid(cap));              // the second walk wants the same count: it fits
        CHECK(cap <= 2 * count + 1024);
    }
    CHECK(scope_near::grown_cap(scope_near::kMaxBandCap) == scope_near::kMaxBandCap);
    CHECK(sizeof(scope_near::BandEntry) == 16);
}

int main()
{
    test_cosine();
    test_in_band();
    test_fold_and_rows();
    test_tail_mask();
    test_arguments();
    test_growth();
    if (g_failed) { printf("orr_scope_near_plan_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("orr_scope_near_plan_selftest: ok\n");
    return 0;
}
