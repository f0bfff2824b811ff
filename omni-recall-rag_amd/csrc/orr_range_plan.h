// orr_range_plan.h -- the rules of a cosine range search (orr_search_range_cosine): for each of up to 64 queries, every live row r
// (of a scope, when one is given) with CosineSimilarity(q_b, e_r) >= min_cosine[b], CosineSimilarity being the reference's
// function (RecallSearchService.cs:69-88) bit for bit and >= C#'s comparison of doubles -- with that cosine, best first.
//
//   arguments     first_invalid: the rules in the order the entry points report them, before a handle is looked at.
//   cosine        scope_near::cosine_of (orr_scope_near_plan.h) of the three exact sums, evaluated on the HOST: the reference's
//                 value.  The guards are the cosine scope's: a row without an embedding is a zero row; a query whose norm is
//                 <= 0, dim 0 and a dim other than the index's give cosine 0 with every row (at_zero) -- no row is walked.
//   screen bound  The streaming int8 screen (K2i, orr_screen.hip) forms dot^ = s1 se_r (I1 + I2 / 254), the exact dot of the
//                 quantised vectors q^ and e^.  By Cauchy-Schwarz
//                     |q.e - dot^| <= |q| |e - e^| + |q - q^| |e^|
//                 and, divided by sqrt(normA) sqrt(normB) (the reference's denominator),
//                     |cos_real - cos^| <= (|q| / sqrt(normA)) re + (|q - q^| / sqrt(normA)) rh,
//                 re = |e - e^| / sqrt(normB) and rh = |e^| / sqrt(normB) as the shadow stores them (binary32, rounded up, a
//                 factor 1.000001 over the fp64 value).  normA is the sum of the binary32-ROUNDED squares, so |q| / sqrt(normA)
//                 is 1 up to 2^-23: the factor 1.0000003 on re.  The reference's dot sums binary32-rounded PRODUCTS
//                 (RecallSearchService.cs:79): each is off by at most 2^-24 of itself, their sum by 2^-24 sum |q_k e_k| <=
//                 2^-24 |q||e|, on the cosine 6e-8 (1 + 2^-23): the 1.2e-7.  The kernel's own roundings -- dot^ in binary64
//                 (three products, one sum), its two reciprocal roots and two more products, each within a few 2^-53 of a value
//                 of size <= 2: < 2^-48 together -- and the underflow of products of rows and queries above the shadow's minima
//                 (D 2^-54, see kI8MinNormB in orr_screen.hip) sit inside the + 1e-9.  This is the expression of
//                 screen_gemv_i8_kernel WITHOUT the score's factor 0.7.  EVERY ROUNDING UPWARD: the expression is a sum of
//                 products of non-negative numbers evaluated in round-to-nearest binary64, seven operations and a root, so the
//                 computed value is below the real one by less than 2^-49 of itself; the result is multiplied by kRoundUp =
//                 1 + 2^-40, which more than restores it.  A bound that is not finite (a row or a query the shadow cannot
//                 vouch for) keeps the pair: screen_keeps.
//   keep          after the exact re-score the device forms its own cosine and drops a pair ONLY when that is finite, below the
//                 threshold, and further from it than scope_near::band_width: device_keeps.  Every other pair goes to the host,
//                 which decides it with cosine_of and >= : no verdict of the device is final at the border.
//   buffers       survivors' buffers and hit lists that were too short grow to grown_cap(count) = count + count / 4 + 1024 and
//                 the launch group runs again: a list is never truncated.
//   order         hits leave by cosine descending as double.CompareTo orders (NaN below everything, -0 equal to +0), ties by
//                 candidate position ascending: before().  A cluster merges its shards' lists by the same order on
//                 (cosine, order_key): merge_lists.
//
// Host-only C++17 except the inlines marked ORR_RANGE_HD, which the kernels share (orr_screen.hip: the RANGE ending of
// screen_gemv_i8_kernel; orr_kernels.hip: range_collect, range_collect_dense); host/orr_range_plan_selftest.cpp checks all of it
// on a machine without a GPU.
#pragma once

#include "orr_scope_near_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ORR_RANGE_HD __host__ __device__
#else
#define ORR_RANGE_HD
#endif

namespace range {

constexpr int32_t kMaxQueries = 64;                   // queries of one call
constexpr int32_t kScreenQ = 4;                       // == orr::kMaxI8ScreenQ: queries of one launch of the screen
constexpr int64_t kDefaultPairCap = 1 << 20;          // "range_pair_cap": pairs of ONE query the call re-scores before it gives up
constexpr int64_t kMaxPairCap = (int64_t)1 << 31;
constexpr int64_t kDefaultBuffer = 8192;              // "range_buffer": entries per query of the survivors' buffers and the lists
constexpr int64_t kMaxBuffer = 65535 * 64;            // one 64-entry workgroup per grid row of the exact re-score
enum Form : int32_t { Auto = 0, Screen = 1, Exact = 2 };   // "range_form"
constexpr double kRoundUp = 1.0 + 0x1p-40;

struct ListEntry {                                    // what the device hands to the host for one kept pair
    int64_t row_id;
    double dot;                                       // the exact dot of the pair
    double norm_b;                                    // the row's exact norm
    uint32_t pos;                                     // the row's position
    uint32_t pad;
};
static_assert(sizeof(ListEntry) == 32, "a list entry is two 16-byte stores");

struct Hit {                                          // orr_range_hit
    int64_t row_id;
    int64_t order_key;
    double cosine;
};

inline bool pair_cap_valid(int64_t v) { return v >= 1 && v <= kMaxPairCap; }
inline bool buffer_valid(int64_t v) { return v >= 1 && v <= kMaxBuffer; }
inline bool form_valid(int64_t v) { return v >= Auto && v <= Exact; }

// The first rule the arguments break, 1 .. 9 in the order the entry points report them, or 0.  The pointer rules hold for
// B > 0 only: B == 0 asks for nothing and writes nothing.  *bad_query: the query whose threshold is NaN (rule 9).
inline int32_t first_invalid(int32_t B, int32_t dim, bool q_null, const double *min_cosine, int32_t max_hits, bool hits_null, bool n_null,
                             bool total_null, int32_t *bad_query = nullptr)
{
    if (B < 0 || B > kMaxQueries) return 1;
    if (dim < 0) return 2;
    if (max_hits < 0) return 3;
    if (B == 0) return 0;
    if (q_null && dim > 0) return 4;
    if (!min_cosine) return 5;
    if (hits_null && max_hits > 0) return 6;
    if (n_null) return 7;
    if (total_null) return 8;
    for (int32_t b = 0; b < B; ++b)
        if (min_cosine[b] != min_cosine[b]) { if (bad_query) *bad_query = b; return 9; }
    return 0;
}

// Every cosine of this query is 0 (RecallSearchService.cs:71-72, :84-85): its hits are all the allowed rows or none.
inline bool at_zero(int32_t dim, int32_t index_dim, double norm_a) { return scope_near::foreign_dim(dim, index_dim) || norm_a <= 0.0; }

// The screen's bound on |cos - cos^| of one pair (derivation above).  re, rh: the row's relative norms; qe = |q - q^| / sqrt(normA).
ORR_RANGE_HD inline double cos_bound(double re, double rh, double qe)
{
    return (1.000001 * (re * 1.0000003 + qe * rh + 1.2e-7) + 1e-9) * kRoundUp;
}

// The screen keeps the pair unless even cos^ + bound stays below the threshold; a sum that is not finite always keeps it.
ORR_RANGE_HD inline bool screen_keeps(double cos_hat, double bound, double t)
{
    const double up = cos_hat + bound;
    if (!(fabs(up) <= 1.7976931348623157e308)) return true;
    return !(up < t);
}

// The device, after the exact re-score, with its own cosine c: dropped only when certainly below the threshold.
ORR_RANGE_HD inline bool device_keeps(double c, double t) { return scope_near::in_band(c, t) || scope_near::verdict(c, t); }

// The capacity a buffer that wanted `count` entries grows to: the measured count and a quarter (the second run wants the same),
// in whole 64-entry groups (the exact re-score's workgroups).  The survivors' buffers end at kMaxBuffer; the exact form's lists,
// which no re-score reads, at kMaxPairCap.
inline int64_t grown_cap(int64_t count, int64_t max_cap = kMaxBuffer)
{
    const int64_t cap = (count + count / 4 + 1024 + 63) / 64 * 64;
    return cap > max_cap ? max_cap : cap;
}
// ... and what a sticky size is used as
inline int64_t buffer_cap(int64_t range_buffer, int64_t max_cap = kMaxBuffer) { return std::min<int64_t>(max_cap, (range_buffer + 63) / 64 * 64); }

// double.CompareTo: -1, 0, 1; NaN equals NaN and lies below every number; -0 equals +0.
inline int compare_to(double a, double b)
{
    if (a < b) return -1;
    if (a > b) return 1;
    if (a == b) return 0;
    if (a != a) return b != b ? 0 : -1;
    return 1;
}

// hit (ca, ka) leaves before hit (cb, kb): the larger cosine, then the smaller key (a position, or an order_key)
inline bool before(double ca, int64_t ka, double cb, int64_t kb)
{
    const int c = compare_to(ca, cb);
    return c != 0 ? c > 0 : ka < kb;
}
inline bool hit_before(const Hit &a, const Hit &b) { return before(a.cosine, a.order_key, b.cosine, b.order_key); }

// The best max_hits of several lists, each in order already, in order: a cluster's answer from its shards'.
inline std::vector<Hit> merge_lists(const std::vector<const std::vector<Hit> *> &lists, int64_t max_hits)
{
    std::vector<Hit> out;
    std::vector<size_t> at(lists.size(), 0);
    while ((int64_t)out.size() < max_hits) {
        int best = -1;
        for (size_t g = 0; g < lists.size(); ++g) {
            if (at[g] >= lists[g]->size()) continue;
            if (best < 0 || hit_before((*lists[g])[at[g]], (*lists[(size_t)best])[at[(size_t)best]])) best = (int)g;
        }
        if (best < 0) break;
        out.push_back((*lists[(size_t)best])[at[(size_t)best]++]);
    }
    return out;
}

}  // namespace range
