// orr_diverse_plan.h -- the rules of a diverse search (orr_search_batch_diverse): the plain search's best `pool` rows of a query,
// compared WITH EACH OTHER, and a greedy pass over them in rank order that keeps `topk` of them.
//
//   pool          what orr_search_batch (orr_search_batch_in_scope with a scope) returns for topk = pool: rows, unrounded fused
//                 scores, order.  max(1, topk) <= pool <= kMaxPool = kSelWidth - 8: the largest take the ladder serves from one
//                 selection list (escalation::initial_kprime: take + 8 <= sel_width); a larger pool would send the search to
//                 run_large_k.  Diversification never looks outside the pool: a query may get fewer than topk rows.
//   cosine        c_ij = CosineSimilarity(e_i, e_j) of RecallSearchService.cs:69-88 on the two stored rows: the HOST's
//                 scope_near::cosine_of(dot_ij, dot_ii, dot_jj) of three sums that are exact on the device (pair_dots_kernel:
//                 products rounded to binary32, a binary64 sum in index order).  A row without an embedding is a zero row.
//   collapse      ranks 0, 1, ...: a member is kept unless collapse_keeps fails against a member already kept, i.e. unless
//                 c >= max_cosine (C#'s >=: a NaN cosine drops nothing); stops at take = max(1, topk) kept.
//   MMR           rank 0 first; then, take - 1 times, the remaining member with the greatest
//                 mmr_value = (lambda * score) - ((1.0 - lambda) * m), binary64, left to right, no contraction, m the greatest
//                 cosine to a kept member (mmr_fold from -inf, NaN skipped; mmr_penalty_cosine: still -inf -> 0).  Values are
//                 ordered by compare_double (C#'s double.CompareTo: NaN below everything); a tie goes to the lower rank.  With
//                 1.0 - lambda == 0.0 the penalty is exactly 0 whatever m is (inf, NaN): lambda = 1 is the plain order.
//   no launch     needs_dots: a pool below 2 members, an index without a dimension, max_cosine = +inf and lambda == 1 read no cosine.
//   arguments     first_invalid: the rules in the order the entry point reports them.
//   pair matrix   mat_index(stride, i, j): out[l][i][j] of orr_index_pair_dots, both halves written.
//   work split    pair_dots_kernel gives one list to a workgroup of kPairThreads threads; thread t owns the pairs
//                 owned_pair(t, 0 .. kPairsPerThread - 1) of the list's pair_count(cnt) pairs (i <= j, row-major upper triangle),
//                 pair_of turns a pair's number into (i, j).
//
// Host-only C++17 except the inlines marked ORR_DIV_HD, which the kernel shares (orr_gemm.hip: pair_dots_kernel);
// host/orr_diverse_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define ORR_DIV_HD __host__ __device__
#else
#define ORR_DIV_HD
#endif

namespace diverse {

enum Mode : int32_t { Collapse = 0, Mmr = 1 };       // ORR_DIVERSE_COLLAPSE, ORR_DIVERSE_MMR

constexpr int32_t kSelWidth = 64;                    // == orr::kSelWidth (orr_api.hip asserts it)
constexpr int32_t kMaxPool = kSelWidth - 8;          // 56
constexpr int32_t kPairThreads = 256;                // threads of the workgroup that owns one list
constexpr int32_t kMaxPairs = kMaxPool * (kMaxPool + 1) / 2;                          // 1596
constexpr int32_t kPairsPerThread = (kMaxPairs + kPairThreads - 1) / kPairThreads;    // 7

inline bool mode_valid(int32_t mode) { return mode == Collapse || mode == Mmr; }
inline bool pool_valid(int32_t pool) { return pool >= 1 && pool <= kMaxPool; }
inline int32_t take_of(int32_t topk) { return topk > 1 ? topk : 1; }                  // Take(Math.Max(1, topK))

// The first rule the arguments break, 1 .. 6 in the order the entry point reports them, or 0.
inline int32_t first_invalid(bool out_null, int32_t topk, int32_t pool, int32_t mode, double param)
{
    if (out_null) return 1;
    if (!pool_valid(pool)) return 2;
    if (take_of(topk) > pool) return 3;
    if (!mode_valid(mode)) return 4;
    if (param != param) return 5;
    if (mode == Mmr && !(param >= 0.0 && param <= 1.0)) return 6;
    return 0;
}

// orr_index_pair_dots: 1 .. 5 in the order it reports them (the positions are looked at once the shard is known)
inline int32_t first_invalid_pairs(bool out_null, int32_t n_lists, bool off_null, bool pos_null, int32_t stride)
{
    if (out_null) return 1;
    if (n_lists < 0) return 2;
    if (stride < 1 || stride > kMaxPool) return 3;
    if (off_null) return 4;
    if (pos_null) return 5;
    return 0;
}

// whether the greedy pass of this call reads any cosine of a pool of n members
inline bool needs_dots(int32_t mode, double param, int32_t n, int32_t index_dim)
{
    if (n < 2 || index_dim <= 0) return false;
    if (mode == Collapse) return !(param == std::numeric_limits<double>::infinity());
    return (1.0 - param) != 0.0;
}

// C#'s double.CompareTo: NaN sorts below every number and equals itself
inline int compare_double(double a, double b)
{
    if (a < b) return -1;
    if (a > b) return 1;
    if (a == b) return 0;
    if (a != a) return (b != b) ? 0 : -1;
    return 1;
}

// ---- the pair matrix and the kernel's work split -----------------------------------------------------------------------------
ORR_DIV_HD inline int64_t mat_index(int32_t stride, int32_t i, int32_t j) { return (int64_t)i * stride + j; }
ORR_DIV_HD inline int32_t pair_count(int32_t cnt) { return cnt * (cnt + 1) / 2; }
ORR_DIV_HD inline int32_t owned_pair(int32_t thread, int32_t slot) { return thread + slot * kPairThreads; }
// pair p of a list of cnt rows, 0 <= p < pair_count(cnt): row i holds the cnt - i pairs (i, i), (i, i + 1), ..., (i, cnt - 1)
ORR_DIV_HD inline void pair_of(int32_t p, int32_t cnt, int32_t *i, int32_t *j)
{
    int32_t r = 0, len = cnt;
    while (p >= len) { p -= len; --len; ++r; }
    *i = r;
    *j = r + p;
}

// ---- the greedy rules ---------------------------------------------------------------------------------------------------------
inline bool collapse_keeps(double c, double max_cosine) { return !(c >= max_cosine); }

inline double mmr_fold(double m, double c) { if (c > m) m = c; return m; }
inline double mmr_penalty_cosine(double m) { return m == -std::numeric_limits<double>::infinity() ? 0.0 : m; }
inline double mmr_value(double lambda, double score, double m)
{
    const double w = 1.0 - lambda;
    if (w == 0.0) return lambda * score;               // the penalty term is exactly 0, whatever m is
    const double gain = lambda * score;
    const double penalty = w * m;
    return gain - penalty;
}

// The pool's n members in rank order, cosine(i, j) their pairwise cosine; picks[] receives the kept ranks in pick order.
// Returns how many were kept (<= take).
template <class Cos>
inline int32_t select_collapse(int32_t n, int32_t take, double max_cosine, Cos cosine, int32_t *picks)
{
    int32_t kept = 0;
    for (int32_t r = 0; r < n && kept < take; ++r) {
        bool keep = true;
        for (int32_t k = 0; k < kept && keep; ++k) keep = collapse_keeps(cosine(r, picks[k]), max_cosine);
        if (keep) picks[kept++] = r;
    }
    return kept;
}

template <class Cos>
inline int32_t select_mmr(int32_t n, int32_t take, double lambda, const double *score, Cos cosine, int32_t *picks)
{
    if (n <= 0 || take <= 0) return 0;
    const double ninf = -std::numeric_limits<double>::infinity();
    std::vector<double> m((size_t)n, ninf);            // each member's fold over the kept ones so far
    std::vector<uint8_t> taken((size_t)n, 0);
    const bool reads = (1.0 - lambda) != 0.0;
    int32_t kept = 0;
    picks[kept++] = 0;
    taken[0] = 1;
    while (kept < take && kept < n) {
        const int32_t last = picks[kept - 1];
        int32_t best = -1;
        double best_v = 0.0;
        for (int32_t r = 0; r < n; ++r) {
            if (taken[(size_t)r]) continue;
            if (reads) m[(size_t)r] = mmr_fold(m[(size_t)r], cosine(r, last));
            const double v = mmr_value(lambda, score[r], mmr_penalty_cosine(m[(size_t)r]));
            if (best < 0 || compare_double(v, best_v) > 0) { best = r; best_v = v; }      // (a tie keeps the lower rank)
        }
        picks[kept++] = best;
        taken[(size_t)best] = 1;
    }
    return kept;
}

}  // namespace diverse
