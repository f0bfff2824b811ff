// orr_mask_plan.h -- the rules of a masked search (orr_search_batch_masked): ONE scope shared by every query of the batch,
// applied as a mask inside the two-stage screen, so that the shadow is streamed once per batch and not once per (query,
// scoped row) pair as the list path of orr_search_batch_scoped does.
//
// The pass (orr_api.hip, run_masked_pass) changes no screening kernel: the mask enters through the per-row scoring constants
// every screen already reads from an array (FusedEpilogue::rowc), and is made exact by one filter behind the screen:
//   resolve    the ids -> one bitmap over the shard's rows (deleted rows left out), live, took = min(live, max(1, limit))
//   clip       n_clip = one past the position of the took-th set bit: the pass runs over rows [0, n_clip)
//   constants  a row whose bit is clear gets {0, kMaskedRecency}: no cosine part and a recency term below every floor
//   floor      the first sample_rows() in-scope rows are re-scored exactly; their k-th best is a lower bound of the final k-th
//              best whatever the scope looks like (the sampled prefix of the unscoped pass is the NEWEST rows: a scope of old
//              rows has none there)
//   screen     the form plan_form picks for (B, dim, n_clip), unchanged
//   filter     mask_survivors drops every buffered entry whose bit is clear (survivor_in_scope below): keep-everything
//              queries, rows with non-finite constants and the hot-tile bypass buffer rows whatever their constants say
//   tail       the exact tail of the two-stage pass; the trailers keep the floor (ORR_CAND_TWO_STAGE, L) and say that `took`
//              scoped rows took part
//
// The ladder of an uncertified query (every rung masked):
//   the pass -> GrowBuffers once (an overflowing buffer was the only reason) -> WiderK (k' x 4 while that fits a selection
//   list) -> ListParts: the scope bitmap cut by position into consecutive parts of at most mask_part_rows set bits, each part a
//   scoped pass of the existing kind with its own first_rung / next_rung ladder step, the parts' records merged as shards in
//   global order are.  ListParts is exact for every input and ends the ladder; it is also what mask_screen = 2 and ineligible
//   passes run, and what lifts scope::kMaxScopeRows for this call.  The ladder is a query's: of the queries a pass leaves
//   uncertified, those whose overflowing buffer larger buffers can hold repeat together, the others take the next rung at once
//   (a NaN query keeps every row: it must not hold back the growth that answers its neighbours).
//
// Statistics (orr_search_stats) of a masked search:
//   passes               every masked pass, and every scoped pass of the list path (one per part and workspace slice)
//   requeried            the queries of every repeat, the step from the screen to the list path included
//   survivors_*          what mask_survivors left (a query whose buffer overflowed keeps the screen's count: the overflow
//                        signal, and what the grown buffers are sized from)
//   buffer_growths       GrowBuffers steps, as for the unscoped search
//   exact_pass_queries   never raised: no masked search runs the pass over all rows in reference arithmetic
//   pass_mode            5 behind a masked screen, 4 behind the list path
//
// Host-only C++17 except survivor_in_scope, which mask_survivors shares (orr_kernels.hip); host/orr_mask_plan_selftest.cpp
// checks all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>

#include "orr_escalation.h"
#include "orr_scope_plan.h"

#if defined(__HIPCC__)
#define ORR_MASK_HD __host__ __device__
#else
#define ORR_MASK_HD
#endif

namespace mask {

// The recency term of a row outside the scope.  Every term of a real pair's score is bounded: |0.7 cos| <= 0.7 (plus the
// screens' error bounds, far below 1), 0 <= 0.2 kw <= 0.2, 0 < 0.1 rec <= 0.1, so a finite floor lies above -2 and a masked
// row's bound, 0.2 kw - 1e30 + (bounds), far below it.  It is FINITE on purpose: fused_epilogue16 turns non-finite row
// constants into "keep everything" and v_max3_f32 drops NaNs; 1e30 is exact enough in fp32 (the fp32 pre-filter converts it)
// and sums of it with the bounded terms never overflow.  Pairs that get past it all the same (a query without a finite floor,
// a row whose int8 constants are not finite, the hot-tile bypass) are removed by mask_survivors.
constexpr double kMaskedRecency = -1.0e30;

// mask_survivors' decision for one buffered entry: the row lies in front of the clip and its bit is set.
ORR_MASK_HD inline bool survivor_in_scope(const uint32_t *bitmap, uint32_t pos, uint64_t n_clip)
{
    return (uint64_t)pos < n_clip && ((bitmap[pos >> 5] >> (pos & 31u)) & 1u) != 0u;
}

// ---- the in-scope sample --------------------------------------------------------------------------------------------------
// m sampled rows cost m exact pairs per query and leave about k took / m survivors (the k-th best of m random rows sits at
// quantile k / m of the scope), so m ~ sqrt(k took) balances the two.  Whole selection lists of 64.  Clamps: at least 4 k rows
// and 256 (a k-th best needs k rows, and a floor from barely k rows keeps a quarter of the scope), at most 65,536 (the
// sample's pairs are re-scored in fp64 from the fp32 master: 64 Ki rows x 256 queries is already 16 M pairs).
constexpr int64_t kMinSampleRows = 256, kMaxSampleRows = 65536;
inline int64_t sample_rows(int32_t topk, int64_t took)
{
    const int64_t k = std::max<int32_t>(1, topk);
    int64_t m = (int64_t)std::ceil(std::sqrt((double)k * (double)std::max<int64_t>(took, 1)));
    m = std::max<int64_t>(m, std::max<int64_t>(kMinSampleRows, 4 * k));
    m = std::min<int64_t>(m, kMaxSampleRows);
    return (m + 63) / 64 * 64;
}

// ---- eligibility and the cost rule ----------------------------------------------------------------------------------------
constexpr int64_t kMinScreenRows = 48 * 4096;      // 48 x orr::kSelSegRows: what plan_form asks of a two-stage pass

// The masked screen needs what a two-stage pass needs, over the clipped rows, and a scope larger than its sample.
inline bool eligible(bool use_cos, int32_t dim, int32_t topk, int32_t sel_width, int64_t n_clip, int two_stage_opt, int64_t took)
{
    if (!use_cos || dim <= 0 || dim % 64 != 0 || two_stage_opt == 0) return false;
    if (std::max<int32_t>(1, topk) > sel_width) return false;
    if (n_clip < kMinScreenRows) return false;
    return took > sample_rows(topk, took);
}

// By bytes the list path reads 4 D per (query, scoped row) pair and the screen about D per row once: the screen would pay
// when 4 B took >= n_clip.  Measured (1M x 3072, one MI355X) that holds for large batches only: a list pass of
// few queries is latency-bound, not byte-bound -- 93 ns per scoped row at B = 1 and 40 ns at B = 8 against 0.72 ns per
// screened row, a factor of 130 and 53 where the byte model says 4 and 32 -- so the masked call already wins from about 6,300
// (B = 1) and 15,000 (B = 8) scoped rows on, not from 250,000 and 31,250.  The rule is therefore the measured one: a scoped
// row of the list path counts as at least kMinRowFactor screened rows, and as 4 B of them from 32 queries on.
constexpr int64_t kMinRowFactor = 128;
inline bool screen_pays(int32_t B, int64_t took, int64_t n_clip)      // max(4 B, 128) took >= n_clip, without the product
{
    const int64_t per = std::max<int64_t>(4 * (int64_t)std::max<int32_t>(B, 1), kMinRowFactor);
    return took >= (std::max<int64_t>(n_clip, 0) + per - 1) / per;
}

enum class Path { Screen, List };
// mask_screen: 0 by the cost rule, 1 whenever eligible, 2 never.
inline Path choose(int mask_screen, bool is_eligible, int32_t B, int64_t took, int64_t n_clip)
{
    if (mask_screen == 2 || !is_eligible) return Path::List;
    if (mask_screen == 1) return Path::Screen;
    return screen_pays(B, took, n_clip) ? Path::Screen : Path::List;
}

// ---- the ladder behind a masked screen ------------------------------------------------------------------------------------
enum class Step { GrowBuffers, WiderK, ListParts };
struct Next {
    Step step = Step::ListParts;
    int64_t kprime = 0;          // k' of the repeat (GrowBuffers, WiderK)
    uint32_t new_cap = 0;        // GrowBuffers: entries per query of the repeat's buffers
};

// The step after a pass that left `again` queries uncertified.  only_overflow: every one of them overflowed its buffer;
// worst: the largest count among them; grown: a GrowBuffers step was already taken for these queries.
inline Next next_step(bool only_overflow, bool grown, uint32_t pass_cap, uint32_t worst, int64_t n_clip, size_t again, int64_t kprime,
                      int32_t sel_width)
{
    Next n;
    n.kprime = kprime;
    if (only_overflow && !grown && escalation::grown_survivor_cap(pass_cap, worst, n_clip, again, &n.new_cap)) {
        n.step = Step::GrowBuffers;
    } else if (kprime * 4 <= sel_width) {
        n.step = Step::WiderK;
        n.kprime = kprime * 4;
    } else {
        n.step = Step::ListParts;
    }
    return n;
}
// GrowBuffers once, WiderK 1 -> 4 -> 16 -> 64 at the longest; then ListParts, whose own ladder is scope::kMaxRungs long.
constexpr int kMaxScreenRepeats = 1 + 3;

// ---- the list path in parts -----------------------------------------------------------------------------------------------
// mask_part_rows: the most scoped rows one part takes (an option so that tests reach several parts on a small shard).
constexpr int64_t kDefaultPartRows = scope::kMaxScopeRows;
inline bool part_rows_valid(int64_t v) { return v >= 1 && v <= (int64_t)scope::kMaxScopeRows; }

inline int64_t part_count(int64_t took, int64_t part_rows) { return took <= 0 ? 0 : (took + part_rows - 1) / part_rows; }
// part j holds the scoped rows of rank [first, last) among the first `took` of the scope
inline std::pair<int64_t, int64_t> part_range(int64_t j, int64_t took, int64_t part_rows)
{
    const int64_t first = std::min(took, j * part_rows);
    return {first, std::min(took, first + part_rows)};
}
// candidate_limit as a part sees it: the call's limit minus the scoped rows of the parts in front
inline int64_t part_limit(int64_t limit, int64_t rows_in_front) { return std::max<int64_t>(0, limit - rows_in_front); }

// The bits of `word` whose rank among the bitmap's set bits lies in [first, last), `before` set bits in front of the word.
ORR_MASK_HD inline uint32_t part_word(uint32_t word, uint64_t before, uint64_t first, uint64_t last)
{
    return scope::clip_word(word, before, last) & ~scope::clip_word(word, before, first);
}

// Queries merged together on the list path: the parts' records of one merge, parts x queries x (K + 1) records of 56 bytes,
// stay within the budget (at least one query).
constexpr size_t kRecordBytes = 56, kMergeBudgetBytes = (size_t)1 << 30;
inline int32_t merge_group(int32_t nq, int64_t parts, int64_t K, size_t budget)
{
    const size_t per_query = (size_t)std::max<int64_t>(parts, 1) * ((size_t)std::max<int64_t>(K, 1) + 1) * kRecordBytes;
    const size_t fit = std::max<size_t>(1, budget / per_query);
    return (int32_t)std::min<size_t>((size_t)std::max<int32_t>(nq, 1), fit);
}

// ---- workspace ------------------------------------------------------------------------------------------------------------
// Queries per masked pass: the survivors' buffers (select_fused halves them down to 8192 entries of 40 bytes per query and no
// further) and the sample's pairs (entry 16, list slot 16, exact dot 8) stay within escalation::kPassWorkspaceBytes.  The one
// shared bitmap costs scope::bitmap_bytes(n_rows) twice on the list path in parts (the scope and the part), whatever the batch.
constexpr size_t kPairBytes = 40;
constexpr uint32_t kMinPassCap = 8192;
inline int32_t screen_slice(int32_t B, int64_t sample)
{
    const size_t per_query = kPairBytes * (size_t)std::max<int64_t>(sample, (int64_t)kMinPassCap);
    const size_t fit = std::max<size_t>(1, escalation::kPassWorkspaceBytes / per_query);
    return (int32_t)std::min<size_t>((size_t)std::max<int32_t>(B, 1), fit);
}

}  // namespace mask
