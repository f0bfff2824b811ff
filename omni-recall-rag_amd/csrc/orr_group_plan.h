// orr_group_plan.h -- the rules of a grouped masked search (orr_search_batch_masked_groups): G scopes, each shared by the
// queries that name it, screened together in ONE pass over the shard's shadow instead of one masked pass per scope.
//
// Each group alone is a masked search (orr_mask_plan.h) and the result of every query is exactly that search's.  What the
// grouped pass (orr_api.hip, run_masked_pass with a GroupScopes) shares between the groups is the stream:
//   resolve    the ids -> G bitmaps (group_off as the offsets of G pseudo-queries), live_g, took_g = min(live_g, max(1, limit))
//   clip       n_clip_g per group; the pass runs over rows [0, n_clip), n_clip the largest clip of a screen group
//   constants  row_consts_grouped: a row keeps its real constants when SOME screen group holds it in front of that group's own
//              clip, else {0, mask::kMaskedRecency}
//   floor      per query the first m_g rows of ITS group are re-scored exactly (scope_compact picks the bitmap per query);
//              samples of different lengths share buffers of max m_g entries, the lists behind a query's count are empty
//   screen     the form plan_form picks for (B, dim, n_clip), unchanged: a row of another group that beats a query's floor IS
//              buffered for that query
//   filter     mask_survivors_grouped: mask::survivor_in_scope against the bitmap and the clip of the query's own group.  This
//              is what makes the call exact
//   tail       the exact tail; the trailer of query b says that took_{group(b)} rows took part
//
// Which groups screen together:
//   used group    named by at least one query, took_g > 0.  ONE used group: the masked call itself, nothing of this header runs
//   m_g           sample_rows() below
//   screen group  a used group with took_g > m_g; the others are list groups and run as a masked call of their own (their
//                 queries as a sub-batch, the results scattered back)
//   grouped pass  eligible (mask::eligible over the largest clip, at least one screen group) and, for mask_screen = 0, paying:
//                 sum over the screen groups of max(max(4 B_g, 128) took_g, kMinCallRows) >= n_clip -- orr_mask_plan.h's
//                 measured rule summed: what each group's own call would cost, counted in screened rows, against one stream;
//                 a call counts as at least kMinCallRows of them (screen_pays below has the measurement).  It inherits that
//                 rule's caveat: both constants were measured at dim 3072 only.  mask_screen = 1 forces the grouped pass
//                 whenever eligible, 2 forbids it.  Without the grouped pass every used group is a masked call of its own.
//
// The ladder of a query the grouped pass leaves uncertified:
//   GrowBuffers  once, for the queries whose only problem was an overflowing buffer that larger buffers can hold: they repeat
//                together with buffers sized from the measured counts.  The size is this CALL's: the counts are inflated by
//                other groups' rows, so neither the lane nor the handle keeps it and no unscoped search inherits it.
//   GroupLadder  every other query, with the rest of its group's uncertified queries, enters the masked call's own ladder for
//                its group (mask::next_step: the masked screen, GrowBuffers, WiderK, ListParts), which is exact and ends.  The
//                driver runs it as a masked call of the group from its resolve on (orr_api.hip, masked_sub_batches, says why).
// So a query sees at most kMaxGroupedPasses grouped passes and then at most 1 + mask::kMaxScreenRepeats masked passes before
// the list path in parts, whose own ladder is scope::kMaxRungs long.
//
// Statistics: pass_mode 6 behind a grouped screen (4 and 5 where a group's own path ran last); survivors_* count what the
// filter left; a grouped GrowBuffers counts in buffer_growths but leaves survivor_capacity alone; exact_pass_queries is never
// raised.
//
// Host-only C++17 (what the kernels share is mask::survivor_in_scope, orr_mask_plan.h's); host/orr_group_plan_selftest.cpp checks
// all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_mask_plan.h"

namespace group {

// A stated cap, not a measurement: it keeps the group bitmaps at 64 x rows / 8 bytes, about 100 MB at 12.5M rows.
constexpr int32_t kMaxGroups = 64;
inline bool groups_valid(int32_t n_groups) { return n_groups >= 1 && n_groups <= kMaxGroups; }
// query_group[b] names a group for every query
inline bool assignment_valid(const int32_t *query_group, int32_t B, int32_t n_groups)
{
    if (!query_group) return false;
    for (int32_t b = 0; b < B; ++b)
        if (query_group[b] < 0 || query_group[b] >= n_groups) return false;
    return true;
}

inline int64_t took_of(int64_t live, int64_t candidate_limit)
{
    return std::min<int64_t>(std::max<int64_t>(live, 0), std::max<int64_t>(1, candidate_limit));
}

// The clip the row constants apply for group g: a group that is no screen group takes no part in them (clip 0).
inline int64_t screen_clip(bool is_screen_group, int64_t n_clip_g) { return is_screen_group ? n_clip_g : 0; }

// Entries per query of the survivors' buffers of a pass over B queries, as select_fused sizes them: the lane's capacity halved
// down to 8192 while B buffers of 40-byte pairs exceed 2 GiB.
inline uint32_t pass_cap(uint32_t survivor_cap, int32_t B)
{
    uint32_t cap = std::max<uint32_t>(survivor_cap, 64u);
    while (cap > mask::kMinPassCap && (size_t)std::max<int32_t>(B, 1) * cap * mask::kPairBytes > ((size_t)2 << 30)) cap >>= 1;
    return cap;
}

// ---- the in-scope sample of a group -------------------------------------------------------------------------------------------
// Two terms.  mask::sample_rows(topk, took_g) is the optimum for the group's own rows: mask_survivors_grouped runs in front of
// the tail, so only in-scope survivors are re-scored.  But the screen buffers pairs from ALL groups' rows -- about
// k sum_took / m_g of them for a query of group g (the k-th best of m random rows sits at quantile k / m) -- and those must fit
// the buffer: the second term keeps that count at or below HALF a buffer, m_g >= 2 k sum_took / pass_cap.  Half is a design
// choice (the estimate is a mean; half a buffer leaves the same again for its spread), not a measurement.
inline int64_t sample_rows(int32_t topk, int64_t took_g, int64_t sum_took, uint32_t pass_cap_entries)
{
    const int64_t k = std::max<int32_t>(1, topk);
    const int64_t cap = std::max<int64_t>(1, (int64_t)pass_cap_entries);
    const int64_t need = (2 * k * std::max<int64_t>(sum_took, 0) + cap - 1) / cap;
    const int64_t m = std::max<int64_t>(mask::sample_rows(topk, took_g), (need + 63) / 64 * 64);
    return std::min<int64_t>(m, mask::kMaxSampleRows);
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------
enum class Role : uint8_t { Unused, Screen, List };
struct GroupIn {
    int64_t took = 0;       // took_of(live_g, candidate_limit)
    int64_t n_clip = 0;     // one past the took-th set bit (0 while took == 0)
    int32_t queries = 0;    // B_g: queries that name the group
};
struct Plan {
    std::vector<Role> role;         // per group
    std::vector<int64_t> sample;    // m_g per group (0: unused)
    int32_t used = 0, screen_groups = 0;
    int32_t only = -1;              // the one used group when used == 1
    int64_t sum_took = 0;           // over the used groups
    int64_t n_clip = 0;             // the largest clip of a screen group
    int64_t max_sample = 0, min_sample = 0;   // over the screen groups
    int64_t min_took = 0;           // over the screen groups
    bool eligible = false;
    bool grouped = false;           // the grouped pass runs for the screen groups' queries
};

inline bool used(const GroupIn &g) { return g.queries > 0 && g.took > 0; }

// sum over the screen groups of max(max(4 B_g, 128) took_g, kMinCallRows) >= n_clip, without overflow (it stops once the sum
// is reached).  The first term is the masked call's rule per group.  The floor is measured (1M x 3072, one
// MI355X): summed without it the rule left two groups of 3,000 rows with four queries each to two masked calls (1.33 ms)
// where the grouped pass took 0.80 ms -- a masked call has a cost of its own whatever its scope (the resolve, two stream
// synchronises, the launches of a pass): no call of any loop measured took less than 0.44 ms, which is 550,000 rows of a
// grouped pass at its 0.80 ns per row.  A call therefore counts as at least 2^19 screened rows.
constexpr int64_t kMinCallRows = (int64_t)1 << 19;
inline bool screen_pays(const std::vector<GroupIn> &groups, const std::vector<Role> &role, int64_t n_clip)
{
    int64_t left = std::max<int64_t>(n_clip, 0);
    for (size_t g = 0; g < groups.size() && left > 0; ++g) {
        if (role[g] != Role::Screen) continue;
        const int64_t per = std::max<int64_t>(4 * (int64_t)std::max<int32_t>(groups[g].queries, 1), mask::kMinRowFactor);
        const int64_t need = (left + per - 1) / per;              // rows of this group that would cover what is left
        if (groups[g].took >= need) return true;
        left -= std::max<int64_t>(per * groups[g].took, kMinCallRows);
    }
    return left <= 0;
}

inline Plan plan(const std::vector<GroupIn> &groups, int32_t topk, uint32_t pass_cap_entries, int mask_screen, bool use_cos,
                 int32_t dim, int32_t sel_width, int two_stage_opt)
{
    Plan p;
    const size_t G = groups.size();
    p.role.assign(G, Role::Unused);
    p.sample.assign(G, 0);
    for (size_t g = 0; g < G; ++g)
        if (used(groups[g])) { p.used += 1; p.only = (int32_t)g; p.sum_took += groups[g].took; }
    if (p.used != 1) p.only = -1;
    if (p.used <= 1) return p;                                      // the masked call itself
    for (size_t g = 0; g < G; ++g) {
        if (!used(groups[g])) continue;
        p.sample[g] = sample_rows(topk, groups[g].took, p.sum_took, pass_cap_entries);
        if (groups[g].took > p.sample[g]) {
            p.role[g] = Role::Screen;
            p.min_took = p.screen_groups == 0 ? groups[g].took : std::min(p.min_took, groups[g].took);
            p.min_sample = p.screen_groups == 0 ? p.sample[g] : std::min(p.min_sample, p.sample[g]);
            p.screen_groups += 1;
            p.n_clip = std::max(p.n_clip, groups[g].n_clip);
            p.max_sample = std::max(p.max_sample, p.sample[g]);
        } else {
            p.role[g] = Role::List;
        }
    }
    // (mask::eligible asks for a scope larger than its sample: every screen group is one, m_g >= mask::sample_rows(topk, took_g))
    p.eligible = p.screen_groups > 0 && mask::eligible(use_cos, dim, topk, sel_width, p.n_clip, two_stage_opt, p.min_took);
    if (mask_screen == 2 || !p.eligible) p.grouped = false;
    else if (mask_screen == 1) p.grouped = true;
    else p.grouped = screen_pays(groups, p.role, p.n_clip);
    return p;
}

// The floor of a grouped pass comes from lists of different fill: the selection that reads only the lists' heads needs
// 8 k non-empty lists of EVERY query (launch_select_final_sample's own threshold), else the full merge is asked for.
inline bool floor_from_heads(int64_t min_sample, int32_t topk, int32_t sel_width)
{
    return min_sample / sel_width >= 8 * (int64_t)std::max<int32_t>(1, topk);
}

// ---- the ladder behind a grouped pass -------------------------------------------------------------------------------------
enum class Step { GrowBuffers, GroupLadder };
struct Next {
    Step step = Step::GroupLadder;
    uint32_t new_cap = 0;        // GrowBuffers: entries per query of the repeat's buffers, this call's own
};
// The step for `again` uncertified queries of one grouped pass.  only_overflow: every one of them overflowed its buffer;
// worst: the largest count among them; grown: they already repeated with grown buffers.
inline Next next_step(bool only_overflow, bool grown, uint32_t pass_cap_entries, uint32_t worst, int64_t n_clip, size_t again)
{
    Next n;
    if (only_overflow && !grown && escalation::grown_survivor_cap(pass_cap_entries, worst, n_clip, again, &n.new_cap))
        n.step = Step::GrowBuffers;
    return n;
}
// The grouped pass and its one repeat with grown buffers; then a group's own masked ladder.
constexpr int kMaxGroupedPasses = 2;
constexpr int kMaxPassesBeforeListParts = kMaxGroupedPasses + 1 + mask::kMaxScreenRepeats;

// ---- workspace ------------------------------------------------------------------------------------------------------------
// Queries per grouped pass: mask::screen_slice with the largest sample.  The G bitmaps cost G x scope::bitmap_bytes(n_rows) twice
// (the resolved slice, which a group's own list path rewrites, and the call's copy).
inline int32_t screen_slice(int32_t B, int64_t max_sample) { return mask::screen_slice(B, max_sample); }

}  // namespace group
