// orr_cluster_group_plan.h -- the host rules of a grouped search over the shards of a cluster
// (orr_cluster_search_batch_in_scopes: several cluster scope handles in one batch, each shared by the queries that name it).
//
// Every shard runs the record form of the grouped call (orr_search_shard_in_scopes) once; the rules of that pass are
// orr_group_plan.h's, the split of the global candidate_limit and the ladder are orr_cluster_scope_plan.h's, the locks of ONE
// handle are orr_cluster_handle_plan.h's.  What several handles in one call add is here:
//   distinct  a handle listed twice is ONE group of the call and is held ONCE: a second shared hold of a mutex behind a waiting
//             writer can deadlock.  The groups of the call are the distinct handles in the order of their first appearance.
//   holds     the parts of all distinct handles, shared, in one strict total order: ascending shard, within a shard ascending
//             part address -- a refinement of chandle::holds' order (ascending shard, the lower address first), so an edit
//             and a grouped search cannot wait for each other in a cycle.
//   splits    one chandle::handle_split per distinct handle: before[d][shard] and took[d][shard] from the handles' own counts.
//   used      a group some query names and of which a row takes part anywhere; the k' of the first rung is
//             cscope::first_rung's for the largest split total among them.
//   route     after the first rung: a certified query is final; every other one repeats through the in-scope cluster ladder of
//             its own group, together with that group's other uncertified queries, in ascending order.
//
// Host-only C++17; host/orr_cluster_group_plan_selftest.cpp checks all of it against brute-force restatements on a machine
// without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_cluster_handle_plan.h"

namespace cgroup {

// ---- distinct handles ----------------------------------------------------------------------------------------------------------
struct Distinct {
    std::vector<int32_t> first;     // [groups]: the index in the call's scopes at which the group's handle appears first
    std::vector<int32_t> group_of;  // [n_scopes]: the group of each listed scope
};
inline Distinct distinct(const std::vector<uintptr_t> &handles)
{
    Distinct d;
    d.group_of.resize(handles.size());
    for (size_t i = 0; i < handles.size(); ++i) {
        int32_t g = -1;
        for (size_t j = 0; j < d.first.size() && g < 0; ++j)
            if (handles[(size_t)d.first[j]] == handles[i]) g = (int32_t)j;
        if (g < 0) { g = (int32_t)d.first.size(); d.first.push_back((int32_t)i); }
        d.group_of[i] = g;
    }
    return d;
}

// ---- the lock order ------------------------------------------------------------------------------------------------------------
struct Hold {
    int32_t shard;
    int32_t group;
};
inline bool operator==(const Hold &a, const Hold &b) { return a.shard == b.shard && a.group == b.group; }

// parts[d][shard]: the addresses of the per-shard scopes of distinct handle d.  All holds are shared.  An address two groups
// share on a shard (two handles never do; the rule does not rely on it) is held once, for the lower group.
inline std::vector<Hold> holds(const std::vector<std::vector<uintptr_t>> &parts)
{
    std::vector<Hold> h;
    const size_t shards = parts.empty() ? 0 : parts[0].size();
    for (size_t s = 0; s < shards; ++s) {
        std::vector<Hold> here;
        for (size_t d = 0; d < parts.size(); ++d) here.push_back(Hold{(int32_t)s, (int32_t)d});
        std::stable_sort(here.begin(), here.end(), [&](const Hold &a, const Hold &b) { return parts[(size_t)a.group][s] < parts[(size_t)b.group][s]; });
        for (size_t i = 0; i < here.size(); ++i)
            if (i == 0 || parts[(size_t)here[i].group][s] != parts[(size_t)here[i - 1].group][s]) h.push_back(here[i]);
    }
    return h;
}

// ---- the split per group ---------------------------------------------------------------------------------------------------------
// live[d][shard] as the handles report it.  false: a part reports no count (orphaned): ORR_ESTATE, nothing is split.
inline bool splits(const std::vector<std::vector<int64_t>> &live, int64_t candidate_limit, std::vector<cscope::Split> &out)
{
    out.assign(live.size(), cscope::Split{});
    for (size_t d = 0; d < live.size(); ++d)
        if (!chandle::handle_split(live[d], candidate_limit, out[d])) return false;
    return true;
}

// ---- the used groups and the first rung ------------------------------------------------------------------------------------------
struct First {
    std::vector<uint8_t> used;      // [groups]
    int32_t n_used = 0, only = -1;  // only: the used group when n_used == 1 (the in-scope cluster call itself)
    int64_t total = 0;              // the largest split total among the used groups: what cscope::first_rung takes
    std::vector<int32_t> ids;       // ascending: the queries of used groups (the others get no row)
};
// query_group[b]: the group (a distinct handle) query b names
inline First first(const std::vector<cscope::Split> &split, const std::vector<int32_t> &query_group)
{
    First f;
    f.used.assign(split.size(), 0);
    for (size_t b = 0; b < query_group.size(); ++b) {
        const size_t g = (size_t)query_group[b];
        if (split[g].total <= 0) continue;
        f.ids.push_back((int32_t)b);
        if (!f.used[g]) { f.used[g] = 1; f.n_used += 1; f.only = (int32_t)g; f.total = std::max(f.total, split[g].total); }
    }
    if (f.n_used != 1) f.only = -1;
    return f;
}

// ---- after the first rung ----------------------------------------------------------------------------------------------------------
// ids (ascending) ran, cert[i] says whether the merge certified ids[i].  again[g]: the queries of group g that repeat through the
// group's own ladder, ascending; a certified query appears nowhere.
inline void route(const std::vector<int32_t> &ids, const std::vector<uint8_t> &cert, const std::vector<int32_t> &query_group,
                  std::vector<std::vector<int32_t>> &again)
{
    for (size_t i = 0; i < ids.size(); ++i)
        if (!cert[i]) again[(size_t)query_group[(size_t)ids[i]]].push_back(ids[i]);
}

}  // namespace cgroup
