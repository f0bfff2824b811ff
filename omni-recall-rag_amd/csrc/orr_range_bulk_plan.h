// orr_range_bulk_plan.h -- the rules of a BULK cosine range search (orr_search_range_cosine_bulk): orr_search_range_cosine's
// contract (orr_range_plan.h) word for word for up to 1024 queries, whose screen is, where it pays, ONE pass of the int8
// screening GEMM (screen_tile16_kernel with the RANGE ending, orr_screen.hip) instead of one stream over the shard per four
// queries.  Whatever screens a query, the answer is what the old call returns on the same queries in slices of 64: a screen
// only decides which pairs are re-scored exactly, the host decides every pair it receives.
//
//   arguments     first_invalid: range::first_invalid's rules in their order, the first one reading 0 .. 1024.
//   which screen  path_of.  A walked query has the SCREEN form where it has it today (stream_applies: "range_form" not 2,
//                 dim % 128 == 0, four queries' two levels within 64 KiB of LDS, the int8 shadow in place, a finite quantisation
//                 error); every other walked query has the EXACT form.  The SCREEN queries go through the GEMM when gemm_shape
//                 holds (dim % 128 == 0 and dim / 64 > 6: the four-wave forms need more K-tiles than their row ring holds) and,
//                 by "range_gemm": 0 -- at least kGemmMinWalked = 65 of them are walked (up to 64 the stream's sixteen passes
//                 are what the old call costs, and the old call's launches are a tested property); 1 -- from one query up;
//                 2 -- never.  Else the stream, four per launch.  The one-level error is finite exactly when the two-level one
//                 is (i8_queries_kernel: both are +inf for a query it cannot bound), so one test serves both screens.
//   the walk      walk_of: the rule the driver runs (range_run, orr_api.hip).  From the queries' exact norms and quantisation
//                 errors: the queries AT ZERO (range::at_zero), the walked ones in their order -- the SCREEN form's, then the
//                 EXACT form's, each ascending --, whether the GEMM screens the former (gemm_takes), and whether the batch is in
//                 that order already and is walked where it lies.
//   launch groups group_queries: as many queries per launch as their survivors' buffers, re-scored dots and lists fit in 2 GiB
//                 (what range_screen_group reserves), in whole queries for the GEMM and in whole launches of four for the
//                 stream.  A launch of more than kQueryTile = 256 queries walks several query tiles.
//   bound         The GEMM multiplies the FIRST query level only: q^ = s1 a, dot^ = se_r s1 I.  range::cos_bound's derivation
//                 holds for any q^ -- it uses |q - q^| and |e^| only -- so the bound is cos_bound(re, rh, qe1) with
//                 qe1 = sqrt(err2_level1) / sqrt(normA), err2_level1 = 1.000001 |q - s1 a|^2 as i8_queries_kernel sums it in
//                 binary64.  ROUNDING BUDGET: the ending evaluates dot^ = (se_r s1) (double)I -- two binary64 products of
//                 exactly representable factors (two binary32 numbers, an int32 with |I| <= 127^2 D < 2^31), where the stream
//                 has three products and a sum -- then the stream's two reciprocal roots and two products, and cos_bound itself
//                 unchanged: one rounding FEWER than the expression the + 1e-9 and kRoundUp were sized for, each still within
//                 2^-53 of a value of size <= 2, < 2^-48 together; the underflow term (D 2^-54) is the row's and the query's
//                 minima's, which are the same.  So the budget covers this evaluation with room to spare.
//   lane map      tile_query_of / tile_row_of: which (query, row) of its wave's 128 x 128 tile element e of accumulator tile
//                 (i, j) of a lane is -- a bijection per lane set, restated here for the host's check against tile16_c_of /
//                 tile16_g_of (orr_epilogue.h).
//
// Host-only C++17; host/orr_range_bulk_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include "orr_range_plan.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace range_bulk {

constexpr int32_t kMaxQueries = 1024;                 // queries of one bulk call
constexpr int32_t kGemmMinWalked = range::kMaxQueries + 1;   // "range_gemm" 0: SCREEN queries walked from which the GEMM screens them
constexpr int32_t kQueryTile = 256;                   // == kScBM: queries of one query tile of the GEMM
constexpr int64_t kGroupBytes = (int64_t)2 << 30;     // what one launch group's buffers may take
constexpr int64_t kPairBytes = 16 + 8 + 32;           // SelEntry + the re-scored dot + range::ListEntry
enum Gemm : int32_t { Auto = 0, Always = 1, Never = 2 };     // "range_gemm"
enum Path : int32_t { ExactForm = 0, Stream = 1, GemmScreen = 2 };

inline bool gemm_valid(int64_t v) { return v >= Auto && v <= Never; }

// range::first_invalid with the first rule reading 0 .. kMaxQueries (rule 9, the NaN threshold, stays the last)
inline int32_t first_invalid(int32_t B, int32_t dim, bool q_null, const double *min_cosine, int32_t max_hits, bool hits_null, bool n_null,
                             bool total_null, int32_t *bad_query = nullptr)
{
    if (B < 0 || B > kMaxQueries) return 1;
    const int32_t head = B < range::kMaxQueries ? B : range::kMaxQueries;
    const int32_t r = range::first_invalid(head, dim, q_null, min_cosine, max_hits, hits_null, n_null, total_null, bad_query);
    if (r != 0) return r;
    for (int32_t b = head; b < B; ++b)
        if (min_cosine[b] != min_cosine[b]) { if (bad_query) *bad_query = b; return 9; }
    return 0;
}

// the shapes: where the streaming screen runs (range_queries takes the int8 images there), and the four-wave forms' condition
inline bool stream_shape(int32_t dim) { return dim > 0 && dim % 128 == 0 && 2 * (int64_t)range::kScreenQ * dim <= 65536; }
inline bool gemm_shape(int32_t dim) { return dim > 0 && dim % 128 == 0 && dim / 64 > 6; }

// a walked query has the SCREEN form (else the EXACT form)
inline bool stream_applies(int32_t dim, bool shadow, bool finite_err, int32_t range_form)
{
    return range_form != range::Exact && stream_shape(dim) && shadow && finite_err;
}

// Whether the walked SCREEN queries of a call, n_screen of them, go through the GEMM.  bulk: the bulk entry point (the old one
// launches what it always launched).
inline bool gemm_takes(int32_t dim, int32_t n_screen, int32_t range_gemm, bool bulk)
{
    if (!bulk || range_gemm == Never || !gemm_shape(dim) || n_screen < 1) return false;
    return range_gemm == Always || n_screen >= kGemmMinWalked;
}

// the path of one walked query
inline Path path_of(int32_t dim, bool shadow, bool finite_err, int32_t n_screen, int32_t range_gemm, int32_t range_form, bool bulk = true)
{
    if (!stream_applies(dim, shadow, finite_err, range_form)) return ExactForm;
    return gemm_takes(dim, n_screen, range_gemm, bulk) ? GemmScreen : Stream;
}

// The walk of one call, both entry points': every query's form and the order the walked ones are put in.
struct Walk {
    std::vector<int32_t> zero;                        // the queries AT ZERO (range::at_zero: no row is walked), ascending
    std::vector<int32_t> perm;                        // the walked queries: the SCREEN form's first, then the EXACT form's, each ascending
    int32_t n_screen = 0;                             // how many of perm have the SCREEN form
    bool gemm = false;                                // the GEMM screens them (gemm_takes); else the stream
    bool in_place = true;                             // perm[p] == p throughout: the batch is walked where it lies
};

// norm_a[b]: query b's exact norm; err2[b]: its two-level quantisation error (+inf where none was taken); shadow: the int8 shadow
// is in place.  Made of range::at_zero, stream_applies and gemm_takes and of nothing else.
inline Walk walk_of(int32_t B, int32_t dim, int32_t index_dim, const double *norm_a, const double *err2, bool shadow, int32_t range_form,
                    int32_t range_gemm, bool bulk)
{
    Walk w;
    std::vector<int32_t> exact;
    for (int32_t b = 0; b < B; ++b) {
        if (range::at_zero(dim, index_dim, norm_a[b])) w.zero.push_back(b);
        else if (stream_applies(index_dim, shadow, std::isfinite(err2[b]), range_form)) w.perm.push_back(b);
        else exact.push_back(b);
    }
    w.n_screen = (int32_t)w.perm.size();
    w.perm.insert(w.perm.end(), exact.begin(), exact.end());
    w.gemm = gemm_takes(index_dim, w.n_screen, range_gemm, bulk);
    for (size_t p = 0; p < w.perm.size(); ++p) w.in_place = w.in_place && w.perm[p] == (int32_t)p;
    return w;
}

// Queries of one launch group at `cap` entries per query: what fits kGroupBytes, in whole units (1: the GEMM; range::kScreenQ:
// the stream's launches), never fewer than one unit.
inline int32_t group_queries(int64_t cap, int32_t unit)
{
    const int64_t per_query = cap * kPairBytes;
    const int64_t fit = (kGroupBytes / per_query) / unit * unit;
    const int64_t q = fit > unit ? fit : unit;
    return (int32_t)(q > kMaxQueries ? (kMaxQueries + unit - 1) / unit * unit : q);
}

// query tiles of a GEMM launch of nq queries (more than one: the rows are re-read, not requested non-temporal)
inline int32_t query_tiles(int32_t nq) { return (nq + kQueryTile - 1) / kQueryTile; }

// ---- the RANGE ending's lane map (screen_tile16_kernel): lane l of a wave is (c, g) = (tile16_c_of(l), tile16_g_of(l)); element e
// of its accumulator tile (i, j) = a[4 (8 i + j) + e] belongs to query 16 i + 4 g + e and row 16 j + c of the wave's tile
constexpr int lane_c(int lane) { return ((((0 - ((lane & 15) >> 2)) & 3) << 2) | (lane & 3)); }
constexpr int lane_g(int lane) { return (0 - (lane >> 4)) & 3; }
constexpr int tile_query_of(int lane, int i, int e) { return 16 * i + 4 * lane_g(lane) + e; }
constexpr int tile_row_of(int lane, int j) { return 16 * j + lane_c(lane); }

}  // namespace range_bulk
