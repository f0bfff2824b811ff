// orr_scope_plan.h -- the rules of a scoped search (orr_search_batch_scoped, orr_search_shard_scoped): which form a pass takes,
// the ladder an uncertified query climbs, how a batch is cut into slices whose workspace stays bounded, what makes a set of
// scope offsets valid, and the clip of a scope bitmap to its first `limit` rows.
//
// A scoped pass never goes through a screen: the rows a caller lists are resolved to positions on the device, kept as one
// bitmap over the shard's rows per query (which removes repeats, gives candidate order, and lets candidate_limit be a prefix
// popcount), and become the entries of the survivors' buffers that the exact tail of the two-stage pass consumes.  The rungs
// of escalation::decide do not apply to it (GrowBuffers asks for larger buffers of a screen, Unfused and Exact run over all
// rows), so the scoped pass has a ladder of its own:
//   Selection    k' <= one selection list: the tail selects k' per query on the device, the trailer carries the cut-off, the
//                host certifies; an uncertified query repeats with k' x 4 while that still fits a list and is below its scope
//   AllRecords   every scoped pair becomes a record with its exact dot and the host finish ranks them: certified by
//                construction, the ladder's end
//
// Host-only C++17 except clip_word, which the compaction kernel shares (orr_kernels.hip); host/orr_scope_plan_selftest.cpp
// checks all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "orr_escalation.h"

#if defined(__HIPCC__)
#define ORR_SCOPE_HD __host__ __device__
#else
#define ORR_SCOPE_HD
#endif

namespace scope {

// The bits of `word` that stay when only the first `limit` set bits of a bitmap take part and `before` set bits lie in
// front of this word: all of them, none, or the lowest limit - before.
ORR_SCOPE_HD inline uint32_t clip_word(uint32_t word, uint64_t before, uint64_t limit)
{
    if (before >= limit) return 0u;
    const uint64_t room = limit - before;
    while ((uint64_t)__builtin_popcount(word) > room) word &= ~(0x80000000u >> __builtin_clz(word));   // drop the highest set bit
    return word;
}

// scope_off[B + 1] (or null: every query owns the whole list) against n_ids listed ids: starts at 0, never decreases,
// ends at n_ids.
inline bool offsets_valid(const uint64_t *scope_off, int32_t B, int64_t n_ids)
{
    if (n_ids < 0 || B < 0) return false;
    if (!scope_off) return true;
    if (scope_off[0] != 0) return false;
    for (int32_t b = 0; b < B; ++b)
        if (scope_off[b + 1] < scope_off[b]) return false;
    return scope_off[B] == (uint64_t)n_ids;
}

enum class Form { Selection, AllRecords, Done };

struct Rung {
    Form form = Form::Done;
    int64_t kprime = 0;          // records per query of the pass
};

// The pass a batch starts with: `take` results asked, the largest scope of the batch holds max_scope rows.
inline Rung first_rung(int32_t take, int64_t max_scope, int32_t sel_width)
{
    const int64_t kprime = escalation::initial_kprime(take, max_scope, sel_width);
    if (kprime > sel_width || kprime >= max_scope) return Rung{Form::AllRecords, std::max<int64_t>(1, max_scope)};
    return Rung{Form::Selection, kprime};
}

// The pass of the queries a pass could not certify; Done: nothing more exact exists (only behind AllRecords).
inline Rung next_rung(const Rung &cur, int64_t max_scope, int32_t sel_width)
{
    if (cur.form != Form::Selection) return Rung{};
    const int64_t wider = cur.kprime * 4;
    if (wider > sel_width || wider >= max_scope) return Rung{Form::AllRecords, std::max<int64_t>(1, max_scope)};
    return Rung{Form::Selection, wider};
}
constexpr int kMaxRungs = 8;     // 1 -> 4 -> 16 -> 64 -> AllRecords at the longest, with room to spare

// Bytes of workspace one (query, scoped row) pair costs a pass: its survivors' entry (16), its exact dot (8), its slot in the
// selection lists (16); AllRecords keeps a record (56) on the device and one on the host side of the copy instead of lists.
constexpr size_t kPairBytesSelection = 40, kPairBytesAllRecords = 24 + 56;
// The tail's one-launch form sorts groups of `group` survivors into lists of 64 slots (orr::finish_survivors_group: 4 for the
// smallest batches, 16, or 0 = whole lists of 64), so a pair's list slots cost 16 x 64 / group bytes there: 280 bytes per pair
// with groups of 4.  A slice is sized by the smallest group any of its sub-batches may get.
inline size_t pair_bytes_selection(int32_t group) { return 24 + (size_t)16 * 64 / (size_t)(group > 0 && group < 64 ? group : 64); }
// The most scoped rows ONE query may bring to a pass: the tail's kernels take a query's buffer as a grid dimension of lists
// of 64 entries, and a grid dimension ends at 65,535.  A scope that resolves to more (and is not clipped below it by
// candidate_limit) is refused with ORR_EINVAL: at that size a scope is a large share of any shard, which is the masked
// screen's job, not this path's.
constexpr uint32_t kMaxScopeRows = 65535u * 64u;
// ... and one scope bitmap per query: a bit per row of the shard
inline size_t bitmap_bytes(int64_t n_rows) { return (size_t)(((std::max<int64_t>(n_rows, 1) + 31) / 32 + 3) / 4 * 4) * 4; }

// Queries whose bitmaps are built together: as many as keep them below the budget (at least one).
inline int32_t bitmap_slice(int32_t B, int64_t n_rows, size_t budget)
{
    const size_t per = bitmap_bytes(n_rows);
    const size_t fit = std::max<size_t>(1, budget / per);
    return (int32_t)std::min<size_t>((size_t)std::max<int32_t>(B, 1), fit);
}

// entries per query of the buffers a slice uses: its largest count in whole selection lists of 64
inline uint32_t slice_cap(uint32_t max_count) { return std::max<uint32_t>(64u, (max_count + 63u) / 64u * 64u); }

// Cuts queries [0, counts.size()) into consecutive slices [first, last) so that queries x slice_cap x pair_bytes stays within
// the budget; a query that exceeds it alone is a slice of its own.  Every query lies in exactly one slice.
inline std::vector<std::pair<int32_t, int32_t>> slice_by_pairs(const std::vector<uint32_t> &counts, size_t pair_bytes, size_t budget)
{
    std::vector<std::pair<int32_t, int32_t>> out;
    const int32_t n = (int32_t)counts.size();
    int32_t first = 0;
    while (first < n) {
        uint32_t worst = counts[(size_t)first];
        int32_t last = first + 1;
        while (last < n) {
            const uint32_t w = std::max(worst, counts[(size_t)last]);
            if ((size_t)(last + 1 - first) * (size_t)slice_cap(w) * pair_bytes > budget) break;
            worst = w;
            ++last;
        }
        out.emplace_back(first, last);
        first = last;
    }
    return out;
}

}  // namespace scope
