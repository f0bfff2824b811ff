// orr_range_plan_selftest -- the rules of orr_range_plan.h on the CPU (no HIP, no GPU): the validity rules in their order, the
// screen's bound against a float64 restatement of the int8 quantisation (Gaussian vectors at three scales, one-hot vectors,
// equal-magnitude vectors: never below the true |cos - cos^|), the screen's and the device's keep rules on both sides of the
// border and at +-0, +-infinity and NaN, the growth rule, the order of hits with ties and NaN, and the merge of 1, 2 and 3
// shard lists against a sort of their union.
// Exit status 0 and a last line "orr_range_plan_selftest: ok" when everything holds; tests/test_range_cosine_cpu.py runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../orr_range_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

static void test_arguments()
{
    const double t[3] = {0.5, -kInf, kInf}, bad[3] = {0.5, kNaN, kNaN};
    int32_t q = -1;
    CHECK(range::first_invalid(3, 128, false, t, 10, false, false, false) == 0);
    const std::vector<double> t64(64, 0.98);
    CHECK(range::first_invalid(64, 128, false, t64.data(), 0, true, false, false) == 0); // totals only: out_hits may be NULL
    CHECK(range::first_invalid(1, 0, true, t, 1, false, false, false) == 0);             // dim 0: q may be NULL
    // each rule alone, then with every later rule broken as well: the first one is reported
    CHECK(range::first_invalid(-1, 128, false, t, 10, false, false, false) == 1);
    CHECK(range::first_invalid(65, -1, true, nullptr, -1, true, true, true) == 1);
    CHECK(range::first_invalid(3, -1, false, t, 10, false, false, false) == 2);
    CHECK(range::first_invalid(3, -1, true, nullptr, -1, true, true, true) == 2);
    CHECK(range::first_invalid(3, 128, false, t, -1, false, false, false) == 3);
    CHECK(range::first_invalid(3, 128, true, nullptr, -1, true, true, true) == 3);
    CHECK(range::first_invalid(3, 128, true, t, 10, false, false, false) == 4);
    CHECK(range::first_invalid(3, 128, true, nullptr, 10, true, true, true) == 4);
    CHECK(range::first_invalid(3, 128, false, nullptr, 10, false, false, false) == 5);
    CHECK(range::first_invalid(3, 128, false, nullptr, 10, true, true, true) == 5);
    CHECK(range::first_invalid(3, 128, false, t, 10, true, false, false) == 6);
    CHECK(range::first_invalid(3, 128, false, bad, 10, true, true, true) == 6);
    CHECK(range::first_invalid(3, 128, false, t, 10, false, true, false) == 7);
    CHECK(range::first_invalid(3, 128, false, bad, 10, false, true, true) == 7);
    CHECK(range::first_invalid(3, 128, false, t, 10, false, false, true) == 8);
    CHECK(range::first_invalid(3, 128, false, bad, 10, false, false, true) == 8);
    CHECK(range::first_invalid(3, 128, false, bad, 10, false, false, false, &q) == 9 && q == 1);
    // B == 0 asks for nothing: only the rules without a pointer hold
    CHECK(range::first_invalid(0, 128, true, nullptr, 10, true, true, true) == 0);
    CHECK(range::first_invalid(0, -1, true, nullptr, 10, true, true, true) == 2);
    CHECK(range::first_invalid(0, 0, true, nullptr, -1, true, true, true) == 3);
    CHECK(range::pair_cap_valid(1) && range::pair_cap_valid((int64_t)1 << 31) && !range::pair_cap_valid(0) && !range::pair_cap_valid(((int64_t)1 << 31) + 1));
    CHECK(range::buffer_valid(1) && range::buffer_valid(range::kMaxBuffer) && !range::buffer_valid(0) && !range::buffer_valid(range::kMaxBuffer + 1));
    CHECK(range::form_valid(0) && range::form_valid(1) && range::form_valid(2) && !range::form_valid(3) && !range::form_valid(-1));
    CHECK(range::at_zero(0, 128, 1.0) && range::at_zero(64, 128, 1.0) && range::at_zero(128, 128, 0.0) && range::at_zero(128, 128, -0.0));
    CHECK(!range::at_zero(128, 128, 1.0) && !range::at_zero(128, 128, kNaN) && !range::at_zero(128, 128, kInf));
}

// ---- the int8 quantisation of orr_screen.hip (i8_quantise_row, i8_rel_norms, i8_queries_kernel), restated in binary64 ------
static float float_ru(double x)
{
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}

struct RowQ { std::vector<int> ie; float se; float re, rh; double nb; };
struct QueryQ { std::vector<int> i1, i2; float s1; double err2, na; };

static RowQ quantise_row(const std::vector<float> &e)
{
    RowQ r;
    float mx = 0.f;
    for (float v : e) mx = std::fmax(mx, std::fabs(v));
    r.se = mx == 0.f ? 0.f : mx / 127.f;
    const float inv = r.se > 0.f ? 1.f / r.se : 0.f;
    double d2 = 0.0, h2 = 0.0;
    r.nb = 0.0;
    for (float v : e) {
        int q = r.se > 0.f ? (int)std::nearbyint(v * inv) : 0;
        q = std::max(-127, std::min(127, q));
        const double hat = (double)r.se * (double)q, dl = (double)v - hat;
        d2 += dl * dl;
        h2 += hat * hat;
        r.ie.push_back(q);
        const float sq = v * v;
        r.nb += (double)sq;
    }
    r.re = r.nb > 0.0 ? float_ru(std::sqrt(d2 / r.nb) * 1.000001) : 0.f;
    r.rh = r.nb > 0.0 ? float_ru(std::sqrt(h2 / r.nb) * 1.000001) : 0.f;
    return r;
}

static QueryQ quantise_query(const std::vector<float> &q)
{
    QueryQ o;
    float mx = 0.f;
    for (float v : q) mx = std::fmax(mx, std::fabs(v));
    o.s1 = mx / 127.f;
    const float s2 = o.s1 / 254.f;
    double e2 = 0.0;
    o.na = 0.0;
    for (float v : q) {
        int a = (int)std::nearbyint(v / o.s1);
        a = std::max(-127, std::min(127, a));
        const double r = (double)v - (double)o.s1 * (double)a;
        int c2 = s2 > 0.f ? (int)std::nearbyint(r / (double)s2) : 0;
        c2 = std::max(-127, std::min(127, c2));
        const double dl = r - (double)o.s1 * ((double)c2 / 254.0);
        e2 += dl * dl;
        o.i1.push_back(a);
        o.i2.push_back(c2);
        const float sq = v * v;
        o.na += (double)sq;
    }
    o.err2 = e2 * 1.000001;
    return o;
}

// the reference's dot (RecallSearchService.cs:77-82): products rounded to binary32, summed in binary64 in index order
static double ref_dot(const std::vector<float> &a, const std::vector<float> &b)
{
    double acc = 0.0;
    for (size_t i = 0; i < a.size(); ++i) {
        const float p = a[i] * b[i];
        acc += (double)p;
    }
    return acc;
}

static double g_worst_share = 0.0;

static void check_pair(const std::vector<float> &q, const std::vector<float> &e)
{
    const QueryQ Q = quantise_query(q);
    const RowQ R = quantise_row(e);
    long long I1 = 0, I2 = 0;
    for (size_t k = 0; k < q.size(); ++k) { I1 += (long long)Q.i1[k] * R.ie[k]; I2 += (long long)Q.i2[k] * R.ie[k]; }
    // the kernel's expression, in its order
    const double isa = 1.0 / std::sqrt(Q.na), isb = R.nb > 0.0 ? 1.0 / std::sqrt(R.nb) : 0.0;
    const double dot_hat = (double)R.se * (double)Q.s1 * ((double)I1 + (double)I2 * (1.0 / 254.0));
    const double cos_hat = dot_hat * isa * isb;
    const double bound = range::cos_bound((double)R.re, (double)R.rh, std::sqrt(Q.err2) * isa);
    const double cos_ref = scope_near::cosine_of(ref_dot(q, e), Q.na, R.nb);
    const double err = std::fabs(cos_ref - cos_hat);
    CHECK(std::isfinite(bound) && bound > 0.0);
    CHECK(err <= bound);
    if (bound > 0.0) g_worst_share = std::max(g_worst_share, err / bound);
    // ... so a pair at or above the threshold is never screened out, whatever the threshold
    CHECK(range::screen_keeps(cos_hat, bound, cos_ref));
    CHECK(range::screen_keeps(cos_hat, bound, std::nextafter(cos_ref, -9.0)));
}

static void test_bound()
{
    std::mt19937_64 rng(11);
    std::normal_distribution<float> g(0.f, 1.f);
    for (int D : {128, 384, 1024}) {
        for (float scale : {1.0f, 0x1p50f, 0x1p-40f}) {
            for (int it = 0; it < 40; ++it) {
                std::vector<float> q((size_t)D), e((size_t)D);
                for (int k = 0; k < D; ++k) { q[(size_t)k] = g(rng) * scale; e[(size_t)k] = g(rng) * scale; }
                check_pair(q, e);
                // a near-duplicate: the regime the call is for
                std::vector<float> near = q;
                for (int k = 0; k < D; ++k) near[(size_t)k] += 0.05f * scale * g(rng);
                check_pair(q, near);
                check_pair(q, q);
            }
        }
        for (int it = 0; it < 20; ++it) {              // one-hot against one-hot and against a Gaussian row
            std::vector<float> a((size_t)D, 0.f), b((size_t)D, 0.f), c((size_t)D);
            a[(size_t)(rng() % (uint64_t)D)] = 3.f;
            b[(size_t)(rng() % (uint64_t)D)] = -0.25f;
            for (int k = 0; k < D; ++k) c[(size_t)k] = g(rng);
            check_pair(a, b); check_pair(a, a); check_pair(a, c); check_pair(c, a);
        }
        for (int it = 0; it < 20; ++it) {              // equal magnitudes, random signs
            std::vector<float> a((size_t)D), b((size_t)D);
            for (int k = 0; k < D; ++k) { a[(size_t)k] = (rng() & 1) ? 0.7f : -0.7f; b[(size_t)k] = (rng() & 1) ? 1e-3f : -1e-3f; }
            check_pair(a, b); check_pair(a, a); check_pair(b, b);
        }
    }
    printf("largest |cos - cos^| as a share of the bound: %.3f\n", g_worst_share);
    CHECK(g_worst_share > 0.01);                       // the bound is not vacuous either
    // every rounding upward: the result is not below the expression in exact arithmetic (long double carries 11 more bits)
    for (int i = 0; i < 1000; ++i) {
        const double re = std::fabs(g(rng)) * 0.01, rh = 1.0 + 0.01 * g(rng), qe = std::fabs(g(rng)) * 1e-4;
        const long double exact = 1.000001L * ((long double)re * 1.0000003L + (long double)qe * (long double)rh + 1.2e-7L) + 1e-9L;
        CHECK((long double)range::cos_bound(re, rh, qe) >= exact);
    }
    // a bound that is not finite keeps the pair whatever the threshold
    CHECK(std::isinf(range::cos_bound(kInf, 0.0, 0.0)) && std::isinf(range::cos_bound(0.0, 1.0, kInf)));
}

static void test_keep()
{
    // the screen: dropped only when cos^ + bound stays below the threshold
    CHECK(range::screen_keeps(0.5, 0.01, 0.51) && range::screen_keeps(0.5, 0.01, 0.5) && range::screen_keeps(0.5, 0.01, -kInf));
    CHECK(!range::screen_keeps(0.5, 0.01, std::nextafter(0.51, 9.0)) && !range::screen_keeps(0.5, 0.01, 0.6) && !range::screen_keeps(0.5, 0.01, kInf));
    CHECK(range::screen_keeps(0.5, kInf, kInf) && range::screen_keeps(kNaN, 0.01, 0.9) && range::screen_keeps(0.5, kNaN, 0.9) && range::screen_keeps(-kInf, kInf, 0.9));
    CHECK(range::screen_keeps(0.0, 0.0, 0.0) && range::screen_keeps(-0.0, 0.0, 0.0) && range::screen_keeps(0.0, 0.0, -0.0));
    CHECK(range::screen_keeps(-kInf, 0.01, 0.0));                                        // -infinity is not finite: kept
    // the device: dropped only when finite, below, and outside the band
    const double band = 0x1p-40;
    for (double t : {-1.0, 0.0, -0.0, 0.3, 0.98, 1.0, 2.0}) {
        CHECK(range::device_keeps(t, t) && range::device_keeps(t + 0.1, t) && range::device_keeps(kInf, t) && range::device_keeps(-kInf, t) && range::device_keeps(kNaN, t));
        CHECK(range::device_keeps(std::nextafter(t, -9.0), t) && range::device_keeps(t - band / 2, t));   // below, but the host decides
        CHECK(!range::device_keeps(t - 4 * band, t) && !range::device_keeps(t - 0.1, t));
    }
    CHECK(range::device_keeps(0.0, -0.0) && range::device_keeps(-0.0, 0.0));
    CHECK(range::device_keeps(0.5, -kInf) && !range::device_keeps(0.5, kInf) && range::device_keeps(kNaN, kInf) && range::device_keeps(kInf, kInf));
    // whatever the device drops, the host would have refused: the device is never final at the border
    std::mt19937_64 rng(3);
    std::uniform_real_distribution<double> u(-1.5, 1.5);
    for (int i = 0; i < 100000; ++i) {
        const double t = u(rng), c = (i & 1) ? t + (u(rng) * 0x1p-38) : u(rng);
        if (!range::device_keeps(c, t)) CHECK(!scope_near::verdict(c, t));
        if (scope_near::verdict(c, t)) CHECK(range::device_keeps(c, t));
    }
}

static void test_growth()
{
    CHECK(range::grown_cap(0) == 1024 && range::grown_cap(1) == 1088 && range::grown_cap(8192) == 11264);
    for (int64_t c : {1, 17, 5000, 8193, 100000, 1 << 20}) {
        const int64_t g = range::grown_cap(c);
        CHECK(g % 64 == 0 && g >= c + c / 4 + 1024 && g < c + c / 4 + 1024 + 64);
    }
    CHECK(range::grown_cap(range::kMaxBuffer) == range::kMaxBuffer && range::grown_cap((int64_t)1 << 30) == range::kMaxBuffer);
    CHECK(range::grown_cap((int64_t)1 << 30, range::kMaxPairCap) == ((int64_t)1 << 30) + ((int64_t)1 << 28) + 1024);
    CHECK(range::grown_cap((int64_t)1 << 31, range::kMaxPairCap) == range::kMaxPairCap);
    CHECK(range::buffer_cap(1) == 64 && range::buffer_cap(16) == 64 && range::buffer_cap(64) == 64 && range::buffer_cap(65) == 128 && range::buffer_cap(8192) == 8192);
    CHECK(range::buffer_cap(range::kMaxBuffer) == range::kMaxBuffer && range::kMaxBuffer % 64 == 0);
}

static void test_order()
{
    // double.CompareTo
    CHECK(range::compare_to(1.0, 2.0) == -1 && range::compare_to(2.0, 1.0) == 1 && range::compare_to(1.0, 1.0) == 0);
    CHECK(range::compare_to(-0.0, 0.0) == 0 && range::compare_to(0.0, -0.0) == 0);
    CHECK(range::compare_to(kNaN, kNaN) == 0 && range::compare_to(kNaN, -kInf) == -1 && range::compare_to(-kInf, kNaN) == 1);
    CHECK(range::compare_to(kInf, 1.0) == 1 && range::compare_to(-kInf, kInf) == -1);
    // cosine descending, then the key ascending
    CHECK(range::before(0.9, 5, 0.8, 1) && !range::before(0.8, 1, 0.9, 5));
    CHECK(range::before(0.9, 1, 0.9, 5) && !range::before(0.9, 5, 0.9, 1) && !range::before(0.9, 5, 0.9, 5));
    CHECK(range::before(0.0, 1, -0.0, 2) && range::before(-0.0, 1, 0.0, 2));             // -0 ties with +0: the position decides
    CHECK(range::before(-kInf, 9, kNaN, 1) && !range::before(kNaN, 1, -kInf, 9) && range::before(kNaN, 1, kNaN, 2));
    // a strict weak order: a sort by it is a sort by (CompareTo descending, key)
    std::mt19937_64 rng(9);
    std::vector<range::Hit> v;
    const double vals[] = {1.0, 0.99, 0.99, 0.5, 0.0, -0.0, -1.0, kNaN, kInf, -kInf};
    for (int i = 0; i < 200; ++i) v.push_back(range::Hit{i, (int64_t)(rng() % 50), vals[rng() % 10]});
    std::sort(v.begin(), v.end(), range::hit_before);
    for (size_t i = 1; i < v.size(); ++i) {
        const int c = range::compare_to(v[i - 1].cosine, v[i].cosine);
        CHECK(c > 0 || (c == 0 && v[i - 1].order_key <= v[i].order_key));
    }
}

static void test_merge()
{
    std::mt19937_64 rng(21);
    const double vals[] = {1.0, 0.999, 0.98, 0.98, 0.98, 0.5, 0.0, -0.0};
    for (int G = 1; G <= 3; ++G) {
        for (int it = 0; it < 50; ++it) {
            std::vector<std::vector<range::Hit>> shard((size_t)G);
            std::vector<range::Hit> all;
            int64_t key = 0;
            for (int g = 0; g < G; ++g) {              // a shard's keys lie behind those of the shards in front
                const int n = (int)(rng() % 40);
                for (int i = 0; i < n; ++i) shard[(size_t)g].push_back(range::Hit{key * 7 + 1, key, vals[rng() % 8]}), ++key;
                std::sort(shard[(size_t)g].begin(), shard[(size_t)g].end(), range::hit_before);
                all.insert(all.end(), shard[(size_t)g].begin(), shard[(size_t)g].end());
            }
            std::sort(all.begin(), all.end(), range::hit_before);
            std::vector<const std::vector<range::Hit> *> lists;
            for (const auto &s : shard) lists.push_back(&s);
            for (int64_t max_hits : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)all.size(), (int64_t)all.size() + 5}) {
                const std::vector<range::Hit> m = range::merge_lists(lists, max_hits);
                CHECK((int64_t)m.size() == std::min<int64_t>(max_hits, (int64_t)all.size()));
                for (size_t i = 0; i < m.size(); ++i)
                    CHECK(m[i].row_id == all[i].row_id && m[i].order_key == all[i].order_key && range::compare_to(m[i].cosine, all[i].cosine) == 0);
            }
        }
    }
    CHECK(range::merge_lists({}, 5).empty());
}

int main()
{
    test_arguments();
    test_bound();
    test_keep();
    test_growth();
    test_order();
    test_merge();
    if (g_failed) { printf("orr_range_plan_selftest: %d checks FAILED\n", g_failed); return 1; }
    printf("orr_range_plan_selftest: ok\n");
    return 0;
}
