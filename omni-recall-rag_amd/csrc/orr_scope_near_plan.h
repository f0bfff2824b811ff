// orr_scope_near_plan.h -- the rules of a cosine scope (orr_scope_create_near): the scope of the live rows r with
// CosineSimilarity(probe_p, e_r) >= min_cosine for EVERY probe (ALL) or for AT LEAST ONE (ANY), CosineSimilarity being the
// reference's function (RecallSearchService.cs:69-88) bit for bit and >= C#'s comparison of doubles.
//
//   cosine        cosine_of(dot, norm_a, norm_b): guard :84-85 (a norm <= 0 gives 0), then dot / (sqrt(norm_a) * sqrt(norm_b)).
//                 The three sums are exact on the device (index order, products rounded to binary32, binary64 accumulators), so
//                 the HOST's value of this expression is the reference's value.  exact_score (orr_api.hip), the kernel and the
//                 band's host decision all call this one function.  A row without an embedding is a zero row: norm_b == 0.
//   verdict       c >= t (NaN is never >= anything).
//   band          The device's sqrt, multiply and divide need not round as the host's do, so the device decides a pair only when
//                 its own c is finite and |c - t| > band_width(c) (in_band is the negation); every other pair goes to the host,
//                 which evaluates cosine_of itself.  Derivation of kBandRel: the device's c is dot / (sa * sb); let u = 2^-53.
//                 HIP documents sqrt(double) at 1 ulp and * and / as IEEE-correct when the code is built without fast-math
//                 (this library is: -fno-fast-math), but the division is a compiler expansion whose bound is not restated for
//                 gfx950, so each of the four operations is charged 4 ulp = 8u here: sa, sb carry (1 +- 8u) each, their product
//                 (1 +- 8u) more, the quotient (1 +- 8u) more: the device's c is within 32u (1 + O(u)) |c| of the real-number
//                 value.  The host's own four roundings (0.5 ulp each) keep it within 4u |c|.  Together < 40u |c| < 2^-47 |c|.
//                 No operand is subnormal: a norm that passed the guard is a sum of binary32 values, >= 2^-149, so sa * sb >=
//                 2^-149, and |dot| < 2^128 * dim.  For |c| <= 2 that is an absolute 2^-46; the band is 2^-40, SIXTY-FOUR times
//                 that, and scales with |c| above 2 (c exceeds 1 only through rounding of the sums, but nothing here relies on
//                 it).  A wide band costs time only: a pair in it is decided by the host, correctly.
//   fold          ALL starts from true and ANDs every probe's verdict in, ANY starts from false and ORs (fold_identity /
//                 fold_verdict).  A fold is SETTLED when a later verdict cannot change it (false under ALL, true under ANY).
//   row           row_state over a row's pairs: the certain verdicts are folded first; settled -> the row is In / Out whatever
//                 its band pairs turn out to be.  Not settled and a pair in the band -> Pending: the certain verdicts folded to
//                 the identity, so the host's fold of the BAND pairs alone, from the identity, is the row's bit.  The kernel
//                 writes a pending row's bit as 1 and lists its band pairs; the host clears the rows whose fold comes out false.
//   tail          the bits at or above n_rows, and the padding words behind them, are clear (tail_mask).  The walk gives a row
//                 past the end dot 0 and norm 0, cosine 0: without the mask those bits would be set whenever 0 >= t.
//   arguments     first_invalid: the rules in the order the entry points report them.
//   foreign dim   dim 0 or a dim other than the index's: every cosine is 0 (:71-72), the scope is all live rows when 0 >= t and
//                 empty otherwise (foreign_dim / all_rows_at_zero): no row is walked.
//   band list     one 16-byte BandEntry per band pair of a pending row; the kernel counts every pair it wanted to list and
//                 stores those below the capacity.  A count above the capacity: the list grows to grown_cap(count) and the walk
//                 runs again -- a scope is never made of a truncated list.
//
// Host-only C++17 except the inlines marked ORR_SNEAR_HD, which the kernels share (orr_kernels.hip: scope_near_tiled,
// scope_near_generic); host/orr_scope_near_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ORR_SNEAR_HD __host__ __device__
#else
#define ORR_SNEAR_HD
#endif

namespace scope_near {

enum Mode : int32_t { All = 0, Any = 1 };
enum RowState : int32_t { Out = 0, In = 1, Pending = 2 };

constexpr int32_t kMaxProbes = 8;                 // == orr::kMaxExactQ: what one walk of the rows carries (orr_kernels.hip asserts it)
constexpr double kBandRel = 0x1p-41;              // band_width = kBandRel * max(2, |c|): 2^-40 for |c| <= 2 (derivation above)
constexpr int64_t kDefaultBandCap = 1 << 16;      // "near_band_cap": 1 MiB of entries; duplicates at the threshold grow it
constexpr int64_t kMaxBandCap = (int64_t)1 << 31; // 8 probes x 2^28 rows
constexpr int kMaxWalks = 4;                      // walks of one fill, the first included, before "the band list kept overflowing"

struct BandEntry {                                // what the kernel hands to the host for one undecided pair
    uint32_t pos;                                 // the row's position
    uint32_t probe;
    double dot;                                   // the exact dot of the pair
};
static_assert(sizeof(BandEntry) == 16, "a band entry is one 16-byte store");

inline bool mode_valid(int32_t mode) { return mode == All || mode == Any; }
inline bool probes_valid(int32_t n_probes) { return n_probes >= 0 && n_probes <= kMaxProbes; }
inline bool band_cap_valid(int64_t cap) { return cap >= 1 && cap <= kMaxBandCap; }

// The first rule the arguments break, 1 .. 6 in the order the entry points report them, or 0.
inline int32_t first_invalid(bool out_null, int32_t n_probes, int32_t dim, bool probes_null, int32_t mode, double min_cosine)
{
    if (out_null) return 1;
    if (!probes_valid(n_probes)) return 2;
    if (dim < 0) return 3;
    if (probes_null && n_probes > 0 && dim > 0) return 4;
    if (!mode_valid(mode)) return 5;
    if (min_cosine != min_cosine) return 6;
    return 0;
}

// RecallSearchService.cs:71-72: a probe of another length than the row's (or of length 0) has cosine 0 with every row.
inline bool foreign_dim(int32_t dim, int32_t index_dim) { return dim == 0 || dim != index_dim; }
// ... and then the scope is every live row or none
inline bool all_rows_at_zero(double min_cosine) { return 0.0 >= min_cosine; }

// RecallSearchService.cs:84-87 from the three exact sums.
ORR_SNEAR_HD inline double cosine_of(double dot, double norm_a, double norm_b)
{
    if (norm_a <= 0.0 || norm_b <= 0.0) return 0.0;
    return dot / (sqrt(norm_a) * sqrt(norm_b));
}

ORR_SNEAR_HD inline bool verdict(double c, double t) { return c >= t; }

ORR_SNEAR_HD inline double band_width(double c)
{
    const double a = fabs(c);
    return kBandRel * (a > 2.0 ? a : 2.0);
}

// The device may not decide this pair: c is not finite, or closer to t than its own arithmetic vouches for.
ORR_SNEAR_HD inline bool in_band(double c, double t)
{
    if (!(fabs(c) <= 1.7976931348623157e308)) return true;       // NaN, +-infinity
    return !(fabs(c - t) > band_width(c));                       // (t = +-infinity: the difference is infinite, never in the band)
}

ORR_SNEAR_HD inline bool fold_identity(int32_t mode) { return mode == All; }
ORR_SNEAR_HD inline bool fold_verdict(bool acc, bool v, int32_t mode) { return mode == All ? (acc && v) : (acc || v); }
ORR_SNEAR_HD inline bool fold_settled(bool acc, int32_t mode) { return acc != fold_identity(mode); }

// A row from the device's cosines of its n pairs (row rule above).
ORR_SNEAR_HD inline int32_t row_state(const double *c, int32_t n, double t, int32_t mode)
{
    bool acc = fold_identity(mode), band = false;
    for (int32_t p = 0; p < n; ++p) {
        if (in_band(c[p], t)) band = true;
        else acc = fold_verdict(acc, verdict(c[p], t), mode);
    }
    if (n == 0) return Out;                                      // no probes: the empty scope in both modes
    if (fold_settled(acc, mode) || !band) return acc ? In : Out;
    return Pending;
}

// The bits of word w (rows 32 w .. 32 w + 31) that are rows of the shard: below n_rows.
ORR_SNEAR_HD inline uint32_t tail_mask(int64_t w, int64_t n_rows)
{
    const int64_t lo = w * 32;
    if (n_rows >= lo + 32) return 0xFFFFFFFFu;
    if (n_rows <= lo) return 0u;
    return 0xFFFFFFFFu >> (uint32_t)(lo + 32 - n_rows);
}

// A pending row's bit, decided by the host: the fold of its band pairs' verdicts (host cosines) from the identity.
inline bool pending_row_in(const double *host_c, int32_t n_band, double t, int32_t mode)
{
    bool acc = fold_identity(mode);
    for (int32_t i = 0; i < n_band; ++i) acc = fold_verdict(acc, verdict(host_c[i], t), mode);
    return acc;
}

// The capacity a list that wanted `count` entries grows to: the measured count and a quarter (the second walk wants the same).
inline int64_t grown_cap(int64_t count)
{
    const int64_t cap = count + count / 4 + 1024;
    return cap > kMaxBandCap ? kMaxBandCap : cap;
}

}  // namespace scope_near
