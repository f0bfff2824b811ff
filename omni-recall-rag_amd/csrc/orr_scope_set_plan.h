// orr_scope_set_plan.h -- the rules of a scope handle (orr_scope): a set of ROWS of one sealed shard kept as a resident bitmap in
// the layout scope_lookup writes (words % 4 == 0, deleted rows left out, bits at or above n_rows clear), with its chunk counts,
// live rows and n_clip_all, so that a search inside it resolves nothing (orr_search_batch_in_scope / _in_scopes).
//
//   time window   rows are in CreatedAt-DESCENDING candidate order, so the rows with from <= ticks < to are one contiguous range
//                 of positions [p0, p1), found by two binary searches in the host mirror of the timestamps (ticks_range); the
//                 range is filled word-wise (range_word) and the deleted rows cleared behind it
//   combine       AND, OR, ANDNOT word by word (combine_word), in place
//   maintenance   a delete clears the newly deleted positions; compaction and insertion move rows, and the library knows how:
//                 destination row d < first keeps its bit, destination row first + r takes the bit of old position src[r], or
//                 none when src[r] < 0 (a new row is in no scope); rows at or above the new row count and padding words are zero
//                 (remap_source / remap_word).  Compaction: first = 0, src = the live positions; insertion: its source list.
//   n_clip_all    one past the last set bit: what a search whose candidate_limit reaches every live row of the scope uses as its
//                 clip without a launch.  The device gets it as mask_clip with took = live (the live-th set bit IS the last one);
//                 n_clip_all below is the host's restatement from the chunk counts.
//
// Host-only C++17 except the word-level inlines, which the kernels share (orr_kernels.hip); host/orr_scope_set_plan_selftest.cpp
// checks all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <utility>

#if defined(__HIPCC__)
#define ORR_SSET_HD __host__ __device__
#else
#define ORR_SSET_HD
#endif

namespace scope_set {

enum Op : int32_t { And = 0, Or = 1, AndNot = 2 };
inline bool op_valid(int32_t op) { return op >= 0 && op <= 2; }

constexpr int32_t kMaxScopes = 64;       // scopes of one orr_search_batch_in_scopes call (group::kMaxGroups)
inline bool scopes_valid(int32_t n) { return n >= 1 && n <= kMaxScopes; }

// The positions [p0, p1) of the rows with from <= created[p] < to; created[0 .. n) never increases.  The interval is
// half-open, so adjacent windows tile; from >= to is empty; INT64_MIN and INT64_MAX are the open ends (to == INT64_MAX keeps
// a row whose ticks are INT64_MAX).
inline std::pair<int64_t, int64_t> ticks_range(const int64_t *created, int64_t n, int64_t from, int64_t to)
{
    if (n <= 0 || from >= to) return {0, 0};
    // first position whose ticks are below `bound` (all rows in front of it are at or above it)
    auto first_below = [&](int64_t bound) {
        return (int64_t)(std::partition_point(created, created + n, [bound](int64_t t) { return t >= bound; }) - created);
    };
    const int64_t p0 = to == std::numeric_limits<int64_t>::max() ? 0 : first_below(to);
    const int64_t p1 = first_below(from);
    return {p0, std::max(p0, p1)};
}

// The bits of word w (rows 32 w .. 32 w + 31) that lie in [p0, p1).
ORR_SSET_HD inline uint32_t range_word(int64_t w, int64_t p0, int64_t p1)
{
    const int64_t lo = w * 32, hi = lo + 32;
    if (p1 <= lo || p0 >= hi || p0 >= p1) return 0u;
    uint32_t m = 0xFFFFFFFFu;
    if (p0 > lo) m &= 0xFFFFFFFFu << (uint32_t)(p0 - lo);
    if (p1 < hi) m &= 0xFFFFFFFFu >> (uint32_t)(hi - p1);
    return m;
}

ORR_SSET_HD inline uint32_t combine_word(uint32_t dst, uint32_t src, int32_t op)
{
    return op == And ? (dst & src) : op == Or ? (dst | src) : (dst & ~src);
}

// The old position whose bit destination row d takes, or -1: none (a new row, or a row at or above the new row count).
ORR_SSET_HD inline int64_t remap_source(int64_t d, int64_t first, int64_t n_new, const int64_t *src)
{
    if (d < 0 || d >= n_new) return -1;
    if (d < first) return d;
    const int64_t s = src[d - first];
    return s < 0 ? -1 : s;
}

ORR_SSET_HD inline uint32_t bit_at(const uint32_t *bitmap, int64_t words, int64_t pos)
{
    return pos >= 0 && pos < words * 32 ? (bitmap[pos >> 5] >> (uint32_t)(pos & 31)) & 1u : 0u;
}

// One destination word of a remapped bitmap (the kernel forms two of them per wave with a ballot over remap_source / bit_at).
inline uint32_t remap_word(const uint32_t *old_bitmap, int64_t old_words, int64_t w, int64_t first, int64_t n_new, const int64_t *src)
{
    uint32_t out = 0;
    for (int b = 0; b < 32; ++b) out |= bit_at(old_bitmap, old_words, remap_source(w * 32 + b, first, n_new, src)) << b;
    return out;
}

// One past the last set bit of a bitmap whose chunk counts (chunk_words words each) exist; 0 for an empty one.
inline int64_t n_clip_all(const uint32_t *bitmap, int64_t words, const uint32_t *chunk_cnt, int32_t n_chunks, int32_t chunk_words)
{
    int32_t c = n_chunks - 1;
    while (c >= 0 && chunk_cnt[c] == 0u) --c;
    if (c < 0) return 0;
    for (int64_t w = std::min<int64_t>(words, (int64_t)(c + 1) * chunk_words) - 1; w >= (int64_t)c * chunk_words; --w)
        if (bitmap[w]) return w * 32 + (32 - __builtin_clz(bitmap[w]));
    return 0;
}

}  // namespace scope_set
