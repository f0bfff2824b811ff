// orr_scope_terms_plan.h -- the rules of a term scope (orr_scope_create_terms): the scope of the live rows whose content contains
// ALL, or ANY, of a list of terms.  The keyword chain of a search gives every distinct term an exact row bitmap in a scope's own
// word layout (words % 4 == 0, bit r & 31 of word r >> 5); a term scope is those bitmaps folded word by word:
//
//   fold          ALL starts from all ones and ANDs every term's word in, ANY starts from zero and ORs (fold_identity /
//                 fold_word).  A term that matched nothing has an all-zero bitmap: it empties ALL and adds nothing to ANY.
//                 Duplicate terms share one bitmap (the chain folds the DISTINCT terms), and x AND x == x OR x == x anyway.
//   tail          the bits at or above n_rows, and the padding words behind them, are clear in a scope (tail_mask).  The fold
//                 always has at least one term, and the chain's own bitmaps are zero there, so the mask changes a word only
//                 if every folded bitmap carried junk in its tail: a guard, which only the selftest can see.
//   arguments     mode is ALL (0) or ANY (1); 0 .. 256 terms (0: the empty scope, folded by nobody); no term is empty and the
//                 offsets never decrease (first_bad_term).
//
// Host-only C++17 except the word-level inlines, which the kernel shares (orr_kernels.hip: scope_terms_combine);
// host/orr_scope_terms_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define ORR_STERMS_HD __host__ __device__
#else
#define ORR_STERMS_HD
#endif

namespace scope_terms {

enum Mode : int32_t { All = 0, Any = 1 };
inline bool mode_valid(int32_t mode) { return mode == All || mode == Any; }

constexpr int32_t kMaxTerms = 256;       // one row bitmap of workspace per distinct term: 256 terms are 320 MB at 10M rows
inline bool terms_valid(int32_t n_terms) { return n_terms >= 0 && n_terms <= kMaxTerms; }

// The first term that is empty or whose offsets decrease, or -1: term t is bytes [term_off[t], term_off[t + 1]).
inline int32_t first_bad_term(const uint32_t *term_off, int32_t n_terms)
{
    for (int32_t t = 0; t < n_terms; ++t)
        if (term_off[t + 1] <= term_off[t]) return t;
    return -1;
}

// What the fold of no term at all is: every bit for ALL, none for ANY.
ORR_STERMS_HD inline uint32_t fold_identity(int32_t mode) { return mode == All ? 0xFFFFFFFFu : 0u; }

// One more term's word folded into the accumulator.
ORR_STERMS_HD inline uint32_t fold_word(uint32_t acc, uint32_t term_word, int32_t mode) { return mode == All ? (acc & term_word) : (acc | term_word); }

// The bits of word w (rows 32 w .. 32 w + 31) that are rows of the shard: below n_rows.
ORR_STERMS_HD inline uint32_t tail_mask(int64_t w, int64_t n_rows)
{
    const int64_t lo = w * 32;
    if (n_rows >= lo + 32) return 0xFFFFFFFFu;
    if (n_rows <= lo) return 0u;
    return 0xFFFFFFFFu >> (uint32_t)(lo + 32 - n_rows);
}

// Word w of the scope of n terms whose words at w are term_words[0 .. n): the kernel's rule for one word, restated on the host.
inline uint32_t scope_word(const uint32_t *term_words, int32_t n, int32_t mode, int64_t w, int64_t n_rows)
{
    uint32_t acc = fold_identity(mode);
    for (int32_t t = 0; t < n; ++t) acc = fold_word(acc, term_words[t], mode);
    return acc & tail_mask(w, n_rows);
}

}  // namespace scope_terms
