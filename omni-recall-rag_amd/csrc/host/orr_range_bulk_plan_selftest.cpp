// orr_range_bulk_plan_selftest -- the rules of orr_range_bulk_plan.h on the CPU (no HIP, no GPU): which screen a walked query
// gets for every combination of shape, shadow, quantisation error, walked count and the two options; the walk plan the driver
// runs (walk_of) for every batch of up to six queries and across the GEMM's threshold; the launch groups against
// the 2 GiB rule; the argument rules with the batch limit of 1024; the screen's bound for the ONE-level query against a float64
// restatement of the quantisation (Gaussian vectors at three scales, one-hot vectors, equal-magnitude vectors: never below the
// true |cos - cos^|); and the ending's lane map, a bijection onto the wave's 128 x 128 tile.
// Exit status 0 and a last line "orr_range_bulk_plan_selftest: ok" when everything holds; tests/test_range_bulk_cpu.py runs it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../orr_range_bulk_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

static void test_paths()
{
    using namespace range_bulk;
    int n_gemm = 0, n_stream = 0, n_exact = 0;
    for (int32_t dim : {70, 128, 384, 448, 512, 3072})
        for (bool shadow : {false, true})
            for (bool finite : {false, true})
                for (int32_t walked : {1, 64, 65, 1024})
                    for (int32_t gemm : {0, 1, 2})
                        for (int32_t form : {0, 1, 2}) {
                            const Path p = path_of(dim, shadow, finite, walked, gemm, form);
                            // which screen: restated from the issue's words, not from the header's helpers
                            const bool shape = dim % 128 == 0 && dim >= 448;
                            const bool enough = gemm == 1 ? walked >= 1 : walked >= 65;
                            const bool takes = shape && gemm != 2 && enough;
                            CHECK(gemm_takes(dim, walked, gemm, true) == takes && !gemm_takes(dim, walked, gemm, false));
                            const Path want = !stream_applies(dim, shadow, finite, form) ? ExactForm : takes ? GemmScreen : Stream;
                            CHECK(p == want);
                            // the old entry point never takes the GEMM, and is otherwise the same
                            CHECK(path_of(dim, shadow, finite, walked, gemm, form, false) == (want == GemmScreen ? Stream : want));
                            n_gemm += p == GemmScreen; n_stream += p == Stream; n_exact += p == ExactForm;
                        }
    CHECK(n_gemm > 0 && n_stream > 0 && n_exact > 0);
    // the SCREEN form: every one of its four conditions on its own (the rule at work is checked through the walk plan below)
    CHECK(stream_applies(128, true, true, 0) && stream_applies(512, true, true, 1) && stream_applies(8192, true, true, 0));
    CHECK(!stream_applies(128, true, true, 2) && !stream_applies(128, false, true, 0) && !stream_applies(128, true, false, 0));
    CHECK(!stream_applies(70, true, true, 0) && !stream_applies(192, true, true, 0) && !stream_applies(8320, true, true, 0) && !stream_applies(0, true, true, 0));
    CHECK(!gemm_shape(448) && gemm_shape(512) && gemm_shape(3072) && !gemm_shape(384) && !gemm_shape(70) && !gemm_shape(128) && !gemm_shape(480) && !gemm_shape(0));
    CHECK(stream_shape(128) && stream_shape(8192) && !stream_shape(8320) && !stream_shape(70));
    CHECK(kGemmMinWalked == 65 && kMaxQueries == 1024 && kQueryTile == 256);
    CHECK(gemm_valid(0) && gemm_valid(1) && gemm_valid(2) && !gemm_valid(3) && !gemm_valid(-1));
    CHECK(query_tiles(1) == 1 && query_tiles(256) == 1 && query_tiles(257) == 2 && query_tiles(1024) == 4);
}

// ---- the walk plan (walk_of), the rule the driver runs: every query in one place, the places path_of's, the order, the layout
static long long g_walks = 0, g_walks_permuted = 0, g_walks_gemm = 0;

static void check_walk(int32_t B, int32_t dim, int32_t index_dim, const std::vector<double> &norm, const std::vector<double> &err, bool shadow, int32_t form,
                       int32_t gemm, bool bulk)
{
    using namespace range_bulk;
    const Walk w = walk_of(B, dim, index_dim, norm.data(), err.data(), shadow, form, gemm, bulk);
    const int32_t nw = (int32_t)w.perm.size();
    bool ok = w.n_screen >= 0 && w.n_screen <= nw && (int32_t)w.zero.size() + nw == B;
    // every query is in exactly one of zero and perm: AT ZERO there, walked here
    std::vector<int> seen((size_t)B, 0);
    for (int32_t b : w.zero) {
        ok = ok && b >= 0 && b < B;
        if (b >= 0 && b < B) { ++seen[(size_t)b]; ok = ok && range::at_zero(dim, index_dim, norm[(size_t)b]); }
    }
    for (int32_t b : w.perm) {
        ok = ok && b >= 0 && b < B;
        if (b >= 0 && b < B) { ++seen[(size_t)b]; ok = ok && !range::at_zero(dim, index_dim, norm[(size_t)b]); }
    }
    for (int v : seen) ok = ok && v == 1;
    CHECK(ok);
    if (!ok) return;
    // a walked query's place is its path's: the SCREEN queries in front, all through the one screen, the EXACT ones behind
    CHECK(w.gemm == gemm_takes(index_dim, w.n_screen, gemm, bulk));
    bool placed = true, ascending = true, identity = true;
    for (int32_t p = 0; p < nw; ++p) {
        const int32_t b = w.perm[(size_t)p];
        const Path path = path_of(index_dim, shadow, std::isfinite(err[(size_t)b]), w.n_screen, gemm, form, bulk);
        placed = placed && path == (p >= w.n_screen ? ExactForm : w.gemm ? GemmScreen : Stream);
        if (p > 0 && p != w.n_screen) ascending = ascending && w.perm[(size_t)(p - 1)] < b;
        identity = identity && b == p;
    }
    for (size_t i = 1; i < w.zero.size(); ++i) ascending = ascending && w.zero[i - 1] < w.zero[i];
    CHECK(placed);
    CHECK(ascending);
    CHECK(w.in_place == identity);
    ++g_walks; g_walks_permuted += !w.in_place; g_walks_gemm += w.gemm;
}

static void test_walk()
{
    // every batch of 0 .. 6 queries, each with a norm > 0 or <= 0 and a finite or an infinite error, asked with the index's dim
    // and with a foreign one, under every setting of the shadow, the two options and the entry point
    for (int32_t index_dim : {70, 128, 512})
        for (int32_t dim : {index_dim, index_dim + 58, 0})
            for (int32_t B = 0; B <= 6; ++B)
                for (int32_t states = 0; states < (1 << (2 * B)); ++states) {
                    std::vector<double> norm((size_t)B), err((size_t)B);
                    for (int32_t b = 0; b < B; ++b) {
                        norm[(size_t)b] = ((states >> (2 * b)) & 1) ? 1.5 + b : (b & 1) ? -1.0 : 0.0;
                        err[(size_t)b] = ((states >> (2 * b + 1)) & 1) ? 1e-6 * (b + 1) : kInf;
                    }
                    for (bool shadow : {false, true})
                        for (int32_t form : {0, 1, 2})
                            for (int32_t gemm : {0, 1, 2})
                                for (bool bulk : {false, true}) check_walk(B, dim, index_dim, norm, err, shadow, form, gemm, bulk);
                }
    CHECK(g_walks > 1000000 && g_walks_permuted > 0 && g_walks_gemm > 0);
    // across kGemmMinWalked: 64 SCREEN queries stream, 65 and 1024 go through the GEMM -- of a bulk call only; one query the
    // shadow cannot bound among 65 leaves 64 for the stream and, unless it is the last, a permuted batch
    using range_bulk::walk_of;
    for (int32_t B : {64, 65, 1024}) {
        const std::vector<double> norm((size_t)B, 2.0), err((size_t)B, 1e-6);
        for (bool bulk : {false, true}) {
            check_walk(B, 512, 512, norm, err, true, 0, 0, bulk);
            const range_bulk::Walk w = walk_of(B, 512, 512, norm.data(), err.data(), true, 0, 0, bulk);
            CHECK(w.n_screen == B && w.in_place && w.zero.empty() && w.gemm == (bulk && B >= 65));
        }
        check_walk(B, 128, 128, norm, err, true, 0, 0, true);
        CHECK(!walk_of(B, 128, 128, norm.data(), err.data(), true, 0, 0, true).gemm);     // no GEMM shape
    }
    for (int32_t at : {0, 64}) {
        const std::vector<double> norm(65, 2.0);
        std::vector<double> err(65, 1e-6);
        err[(size_t)at] = kNaN;                        // not finite either
        check_walk(65, 512, 512, norm, err, true, 0, 0, true);
        const range_bulk::Walk w = walk_of(65, 512, 512, norm.data(), err.data(), true, 0, 0, true);
        CHECK(w.n_screen == 64 && !w.gemm && w.perm[64] == at && w.in_place == (at == 64));
    }
}

static void test_groups()
{
    using namespace range_bulk;
    static_assert(kPairBytes == 56, "an entry, a dot, a list entry");
    for (int64_t cap : {(int64_t)64, (int64_t)8192, (int64_t)11264, (int64_t)1 << 20, range::kMaxBuffer}) {
        for (int32_t unit : {1, (int32_t)range::kScreenQ}) {
            const int32_t q = group_queries(cap, unit);
            CHECK(q >= unit && q % unit == 0 && q <= kMaxQueries);
            // the group fits 2 GiB, unless it is the single unit every call is owed
            CHECK(q == unit || (int64_t)q * cap * kPairBytes <= kGroupBytes);
            // ... and is the largest that does, short of the call's limit
            CHECK(q == kMaxQueries || (int64_t)(q + unit) * cap * kPairBytes > kGroupBytes);
            // the stream's groups are the cosine range search's own: max(4, (2 GiB / per_query) / 4 * 4), beyond 1024 no call asks
            if (unit == range::kScreenQ) {
                const int64_t old_fit = std::max<int64_t>(range::kScreenQ, (((int64_t)2 << 30) / (cap * 56)) / range::kScreenQ * range::kScreenQ);
                CHECK(q == std::min<int64_t>(old_fit, kMaxQueries));
            }
        }
    }
    CHECK(group_queries(8192, 1) == 1024);                                      // the default buffer: the whole call in one launch
    CHECK(group_queries(range::kMaxBuffer, 1) == 9 && group_queries(range::kMaxBuffer, 4) == 8);
    CHECK(group_queries((int64_t)1 << 20, 1) == 36);
}

static void test_arguments()
{
    using range_bulk::first_invalid;
    std::vector<double> t(1025, 0.9);
    int32_t q = -1;
    // the first rule with B in {-1, 0, 1024, 1025}, alone and with every later rule broken as well
    CHECK(first_invalid(-1, 128, false, t.data(), 10, false, false, false) == 1);
    CHECK(first_invalid(-1, -1, true, nullptr, -1, true, true, true) == 1);
    CHECK(first_invalid(0, 128, true, nullptr, 10, true, true, true) == 0);
    CHECK(first_invalid(0, -1, true, nullptr, 10, true, true, true) == 2);
    CHECK(first_invalid(0, 0, true, nullptr, -1, true, true, true) == 3);
    CHECK(first_invalid(1024, 128, false, t.data(), 10, false, false, false) == 0);
    CHECK(first_invalid(1025, 128, false, t.data(), 10, false, false, false) == 1);
    CHECK(first_invalid(1025, -1, true, nullptr, -1, true, true, true) == 1);
    CHECK(first_invalid(65, 128, false, t.data(), 10, false, false, false) == 0);      // (the old call's ORR_EINVAL)
    // the later rules in their order, at a batch beyond the old limit
    for (int32_t B : {1, 64, 65, 1024}) {
        CHECK(first_invalid(B, -1, true, nullptr, -1, true, true, true) == 2);
        CHECK(first_invalid(B, 128, true, nullptr, -1, true, true, true) == 3);
        CHECK(first_invalid(B, 128, true, nullptr, 10, true, true, true) == 4);
        CHECK(first_invalid(B, 128, false, nullptr, 10, true, true, true) == 5);
        CHECK(first_invalid(B, 128, false, t.data(), 10, true, true, true) == 6);
        CHECK(first_invalid(B, 128, false, t.data(), 10, false, true, true) == 7);
        CHECK(first_invalid(B, 128, false, t.data(), 10, false, false, true) == 8);
        CHECK(first_invalid(B, 128, false, t.data(), 0, true, false, false) == 0);     // totals only
        CHECK(first_invalid(B, 0, true, t.data(), 1, false, false, false) == 0);       // dim 0: q may be NULL
        // a NaN threshold: the last rule, reported with its query -- the first one, wherever it stands
        for (int32_t at : {0, B / 2, B - 1}) {
            std::vector<double> bad = t;
            bad[(size_t)at] = kNaN;
            bad[(size_t)(B - 1)] = kNaN;
            q = -1;
            CHECK(first_invalid(B, 128, false, bad.data(), 10, false, false, false, &q) == 9 && q == at);
            CHECK(first_invalid(B, 128, false, bad.data(), 10, false, false, true) == 8);
        }
    }
    // agreement with the old rules wherever both speak
    for (int32_t B : {-1, 0, 1, 64})
        CHECK(first_invalid(B, 128, false, t.data(), 10, false, false, false) == range::first_invalid(B, 128, false, t.data(), 10, false, false, false));
}

// ---- the int8 quantisation of orr_screen.hip (i8_quantise_row, i8_rel_norms, i8_queries_kernel), restated in binary64 ------
static float float_ru(double x)
{
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}

struct RowQ { std::vector<int> ie; float se; float re, rh; double nb; };
struct QueryQ { std::vector<int> i1; float s1; double err1, err2, na; };

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

// the first level only: q^ = s1 a, err1 = 1.000001 |q - q^|^2; the second level's error beside it (what the stream charges)
static QueryQ quantise_query(const std::vector<float> &q)
{
    QueryQ o;
    float mx = 0.f;
    for (float v : q) mx = std::fmax(mx, std::fabs(v));
    o.s1 = mx / 127.f;
    const float s2 = o.s1 / 254.f;
    double e1 = 0.0, e2 = 0.0;
    o.na = 0.0;
    for (float v : q) {
        int a = (int)std::nearbyint(v / o.s1);
        a = std::max(-127, std::min(127, a));
        const double r = (double)v - (double)o.s1 * (double)a;
        e1 += r * r;
        int c2 = s2 > 0.f ? (int)std::nearbyint(r / (double)s2) : 0;
        c2 = std::max(-127, std::min(127, c2));
        const double dl = r - (double)o.s1 * ((double)c2 / 254.0);
        e2 += dl * dl;
        o.i1.push_back(a);
        const float sq = v * v;
        o.na += (double)sq;
    }
    o.err1 = e1 * 1.000001;
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
static int g_two_level_fails = 0;

static void check_pair(const std::vector<float> &q, const std::vector<float> &e)
{
    const QueryQ Q = quantise_query(q);
    const RowQ R = quantise_row(e);
    long long I = 0;
    for (size_t k = 0; k < q.size(); ++k) I += (long long)Q.i1[k] * R.ie[k];
    CHECK(I > -((long long)1 << 31) && I < ((long long)1 << 31));           // the accumulator is an int32
    // the ending's expression, in its order
    const double isa = 1.0 / std::sqrt(Q.na), isb = R.nb > 0.0 ? 1.0 / std::sqrt(R.nb) : 0.0;
    const double dot_hat = (double)R.se * (double)Q.s1 * (double)(int)I;
    const double cos_hat = dot_hat * isa * isb;
    const double qe1 = std::sqrt(Q.err1) * isa;
    const double bound = range::cos_bound((double)R.re, (double)R.rh, qe1);
    const double cos_ref = scope_near::cosine_of(ref_dot(q, e), Q.na, R.nb);
    const double err = std::fabs(cos_ref - cos_hat);
    CHECK(std::isfinite(bound) && bound > 0.0);
    CHECK(err <= bound);
    if (bound > 0.0) g_worst_share = std::max(g_worst_share, err / bound);
    CHECK(range::screen_keeps(cos_hat, bound, cos_ref));
    CHECK(range::screen_keeps(cos_hat, bound, std::nextafter(cos_ref, -9.0)));
    // the two-level error is the smaller one: charging it for the one-level product would not be a bound in general
    CHECK(Q.err2 <= Q.err1);
    if (err > range::cos_bound((double)R.re, (double)R.rh, std::sqrt(Q.err2) * isa)) ++g_two_level_fails;
}

static void test_bound()
{
    std::mt19937_64 rng(17);
    std::normal_distribution<float> g(0.f, 1.f);
    for (int D : {128, 512, 1024}) {
        for (float scale : {1.0f, 0x1p50f, 0x1p-40f}) {
            for (int it = 0; it < 40; ++it) {
                std::vector<float> q((size_t)D), e((size_t)D);
                for (int k = 0; k < D; ++k) { q[(size_t)k] = g(rng) * scale; e[(size_t)k] = g(rng) * scale; }
                check_pair(q, e);
                std::vector<float> near = q;               // a near-duplicate: the regime the call is for
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
    printf("largest |cos - cos^| as a share of the one-level bound: %.3f; pairs the two-level error would not have covered: %d\n",
           g_worst_share, g_two_level_fails);
    CHECK(g_worst_share > 0.01);                       // the bound is not vacuous either
    CHECK(std::isinf(range::cos_bound(0.0, 1.0, kInf)) && range::screen_keeps(0.3, range::cos_bound(0.0, 1.0, kInf), 0.99));
    CHECK(range::screen_keeps(kNaN, 0.01, 0.9));
}

static void test_lane_map()
{
    using namespace range_bulk;
    std::vector<int> seen(128 * 128, 0);
    for (int lane = 0; lane < 64; ++lane) {
        CHECK(lane_c(lane) >= 0 && lane_c(lane) < 16 && lane_g(lane) >= 0 && lane_g(lane) < 4);
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j)
                for (int e = 0; e < 4; ++e) {
                    const int q = tile_query_of(lane, i, e), r = tile_row_of(lane, j);
                    CHECK(q >= 0 && q < 128 && r >= 0 && r < 128);
                    if (q >= 0 && q < 128 && r >= 0 && r < 128) ++seen[(size_t)q * 128 + (size_t)r];
                }
    }
    bool once = true;
    for (int v : seen) once = once && v == 1;
    CHECK(once);                                       // every (query, row) of the wave tile exactly once
    // a lane's 8 rows and 32 queries
    CHECK(tile_row_of(0, 0) == 0 && tile_row_of(0, 7) == 112 && tile_query_of(0, 0, 0) == 0 && tile_query_of(0, 7, 3) == 115);
    CHECK(lane_c(4) == 12 && lane_c(12) == 4 && lane_c(8) == 8 && lane_g(16) == 3 && lane_g(32) == 2 && lane_g(48) == 1);
}

int main()
{
    test_paths();
    test_walk();
    test_groups();
    test_arguments();
    test_bound();
    test_lane_map();
    if (g_failed) { printf("orr_range_bulk_plan_selftest: %d checks FAILED\n", g_failed); return 1; }
    printf("orr_range_bulk_plan_selftest: ok\n");
    return 0;
}
