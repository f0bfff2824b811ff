// orr_cluster_handle_plan.h -- the host rules of a cluster scope handle (orr_cluster_scope: one orr_scope per shard of one
// sealed cluster) and of the search inside one (orr_cluster_search_batch_in_scope).
//
// The device work is the single shard's (orr_scope_*, the masked shard form); what the cluster level adds is small and lives here:
//   row_ids   the ids come back in the global candidate order -- shard 0's, then shard 1's, ... -- so shard g writes at the sum
//             of the live counts of the shards in front of it; when the sum over all shards exceeds cap nothing is written at
//             all (the count is still reported): nothing lands beyond cap.
//   pair      combine takes two scopes of ONE cluster, both alive, with a part on every shard.
//   holds     the locks of one call over all shards, in the order every call takes them: ascending shard; within a shard the
//             single shard's rule (dst exclusive, src shared, the lower address first, src == dst one exclusive hold).  Two
//             calls that follow it cannot wait for each other in a cycle.
//   split     the search reads every shard's live count from its handle -- no count step -- and splits the global
//             candidate_limit with cscope::split_limit, which is NOT restated here: handle_split hands it the counts and
//             refuses the count of an orphaned part (-1).
//
// Host-only C++17; host/orr_cluster_handle_plan_selftest.cpp checks all of it against brute-force restatements on a machine
// without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_cluster_scope_plan.h"

namespace chandle {

// ---- row_ids ---------------------------------------------------------------------------------------------------------------
struct RowIdPlan {
    std::vector<int64_t> offset;    // [shards]: where shard g's ids start in out_ids
    int64_t total = 0;              // *out_n
    bool fits = false;              // total <= cap: the shards write; else ORR_EINVAL after *out_n is set, nothing written
};
inline RowIdPlan row_id_plan(const std::vector<int64_t> &live, int64_t cap)
{
    RowIdPlan p;
    p.offset.resize(live.size());
    for (size_t g = 0; g < live.size(); ++g) {
        p.offset[g] = p.total;
        p.total += live[g] > 0 ? live[g] : 0;
    }
    p.fits = cap >= 0 && p.total <= cap;
    return p;
}

// ---- combine: the pair -------------------------------------------------------------------------------------------------------
enum class Pair { Ok, Orphaned, OtherCluster, Shards };
// cluster_*: the owning cluster of each scope (null: orphaned); parts_*: the per-shard scopes each holds
inline Pair pair_valid(const void *cluster_dst, const void *cluster_src, size_t parts_dst, size_t parts_src)
{
    if (!cluster_dst || !cluster_src) return Pair::Orphaned;
    if (cluster_dst != cluster_src) return Pair::OtherCluster;
    if (parts_dst != parts_src || parts_dst == 0) return Pair::Shards;
    return Pair::Ok;
}

// ---- the lock order ----------------------------------------------------------------------------------------------------------
struct Hold {
    int32_t shard;
    int32_t which;                  // 0: dst's part, 1: src's part
    bool exclusive;
};
inline bool operator==(const Hold &a, const Hold &b) { return a.shard == b.shard && a.which == b.which && a.exclusive == b.exclusive; }

// dst[g], src[g]: the addresses of the per-shard scopes.  src empty: a call on one scope (add_ids: dst_exclusive; a search or
// row_ids: shared).  With src, dst is held exclusively and src shared (combine).
inline std::vector<Hold> holds(const std::vector<uintptr_t> &dst, const std::vector<uintptr_t> &src, bool dst_exclusive)
{
    std::vector<Hold> h;
    for (size_t g = 0; g < dst.size(); ++g) {
        const Hold d{(int32_t)g, 0, dst_exclusive || !src.empty()};
        if (src.empty() || src[g] == dst[g]) { h.push_back(d); continue; }
        const Hold s{(int32_t)g, 1, false};
        if (dst[g] < src[g]) { h.push_back(d); h.push_back(s); }
        else { h.push_back(s); h.push_back(d); }
    }
    return h;
}

// ---- the split from handle-reported counts -----------------------------------------------------------------------------------
// false: a part reports no count (orphaned, -1): the call is ORR_ESTATE and nothing is split
inline bool handle_split(const std::vector<int64_t> &live, int64_t candidate_limit, cscope::Split &out)
{
    for (int64_t l : live)
        if (l < 0) return false;
    out = cscope::split_limit(live, candidate_limit);
    return true;
}

}  // namespace chandle
