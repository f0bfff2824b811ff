// orr_cluster_per_key_plan.h -- what a cluster adds to the per-key search (orr_cluster_search_batch_per_key).  The answer, the
// rounds, the walk and the union table are the single index's (orr_per_key_plan.h: State, walk_round, build_table, take_of); an
// order key is (shard, position) by cdiverse::locate (orr_cluster_diverse_plan.h); the split of a limit over scoped rows is
// cscope::split_limit (orr_cluster_scope_plan.h).  The rules that are new:
//
//   gather     the members of a round's pools are order keys of the whole cluster.  gather_plan gives every shard the local
//              positions of ITS members (in query, then rank order) and the pool slot each answers, so a shard reads the keys of
//              its own rows with one keys_gather and a shard without a member launches nothing.  A key outside every shard is an
//              error (Gather::ok false), never a guess; an empty shard holds no key.
//   seen       a query's seen set S is kept as order keys.  seen_of_shard hands shard g the pairs (slot, key - base_g) of the
//              keys it holds; a key of another shard is passed over, so no shard clears a bit for a row it does not hold.
//   closed     a key closes CLUSTER-WIDE: the union table of a slice goes to every shard as it is (per_key::build_table), because
//              the rows of one key may lie on any shard.  (Nothing to compute: the rule is that there is no per-shard table.)
//   shares     the frozen candidate set of round 1 on shard g.  Without a scope: the rows below prefix_rows(), the global
//              candidate_limit prefix clipped to the shard with the deleted rows in front of and inside it not counted (the
//              arithmetic of the plain search's participating rows).  With a scope: shard g's took of cscope::split_limit over
//              the parts' live counts; scope_share says whether the part is empty, taken whole or clipped at its took-th bit.
//   holds      the keys' parts and the scope's parts are held shared in one total order: ascending shard, within a shard the
//              lower address first (the order of cgroup::holds and chandle::holds).  They are taken behind the lanes.
//
// Host-only C++17; host/orr_cluster_per_key_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_cluster_diverse_plan.h"
#include "orr_cluster_scope_plan.h"
#include "orr_per_key_plan.h"

namespace cper_key {

// ---- which shard gathers which members -----------------------------------------------------------------------------------------
struct Gather {
    bool ok = true;                                 // false: bad_key of query bad_query lies outside every shard; nothing else is set
    int32_t bad_query = -1;
    int64_t bad_key = 0;
    std::vector<std::vector<int64_t>> pos;          // [shards] the local positions shard g reads, in (query, rank) order
    std::vector<std::vector<int32_t>> at;           // [shards] the slot i * pool + j of the round's arrays each position answers
};

// keys[i * pool + j], j < cnt[i]: the order keys of the round's query i in rank order.
inline Gather gather_plan(const std::vector<int64_t> &base, const std::vector<int64_t> &rows, int32_t nq, int32_t pool, const int64_t *keys,
                          const int32_t *cnt)
{
    Gather g;
    g.pos.assign(base.size(), {});
    g.at.assign(base.size(), {});
    for (int32_t i = 0; i < nq; ++i)
        for (int32_t j = 0; j < cnt[i] && j < pool; ++j) {
            const int64_t key = keys[(size_t)i * (size_t)pool + (size_t)j];
            cdiverse::Place pl{-1, -1};
            if (!cdiverse::locate(base, rows, key, &pl)) {
                Gather bad;
                bad.ok = false; bad.bad_query = i; bad.bad_key = key;
                return bad;
            }
            g.pos[(size_t)pl.shard].push_back(pl.pos);
            g.at[(size_t)pl.shard].push_back(i * pool + j);
        }
    return g;
}

// ---- the seen positions of one shard --------------------------------------------------------------------------------------------
struct Seen {
    std::vector<int64_t> pos;                       // local positions on the shard
    std::vector<int32_t> slot;                      // the slice's slot each belongs to
};

// seen[s]: the order keys slot s has seen.  The shard holds the order keys base .. base + rows - 1.
inline Seen seen_of_shard(int64_t base, int64_t rows, const std::vector<const std::vector<int64_t> *> &seen)
{
    Seen out;
    for (size_t s = 0; s < seen.size(); ++s)
        for (int64_t key : *seen[s])
            if (rows > 0 && key >= base && key - base < rows) { out.pos.push_back(key - base); out.slot.push_back((int32_t)s); }
    return out;
}

// ---- the shares of the limit ---------------------------------------------------------------------------------------------------
// Without a scope.  Rows of a shard that take part: the global candidate prefix clipped to the shard.  Deleted rows do not count:
// the prefix ends behind the shard's local_live-th live row.  row_base: rows in front of the shard; dead_before: deleted rows
// among them; dead[0 .. n_dead): the shard's deleted positions, ascending.
inline int64_t prefix_rows(int64_t candidate_limit, int64_t row_base, int64_t dead_before, int64_t n_rows, const int64_t *dead, size_t n_dead)
{
    const int64_t limit = std::max<int64_t>(1, candidate_limit);     // Take(Math.Max(1, maxCount))
    const int64_t local_live = limit - (row_base - dead_before);
    if (local_live <= 0) return 0;
    int64_t p = local_live;                                          // smallest p with p - dead(< p) == local_live
    for (size_t i = 0; i < n_dead; ++i) {
        if (dead[i] < p) ++p; else break;
        if (p >= n_rows) break;
    }
    return std::min<int64_t>(p, n_rows);
}

// With a scope.  What shard g does with its part of the scope when its share of the limit is split.took[g] of its live rows.
enum class Part { Empty, Whole, Clipped };          // Clipped: the part ends behind its took-th set bit (mask_clip)
struct Share {
    Part part;
    int64_t took;
};
inline Share scope_share(const cscope::Split &split, int32_t g, int64_t live)
{
    const int64_t took = split.took[(size_t)g];
    if (took <= 0) return Share{Part::Empty, 0};
    return Share{took < live ? Part::Clipped : Part::Whole, took};
}

// ---- the order of the holds ----------------------------------------------------------------------------------------------------
struct Hold {
    int32_t shard;
    int32_t which;                                  // 0: the keys' part, 1: the scope's part
};
inline bool operator==(const Hold &a, const Hold &b) { return a.shard == b.shard && a.which == b.which; }

// keys[g], scope[g]: the addresses of the per-shard parts; scope empty: a call without a scope.  All holds are shared.
inline std::vector<Hold> holds(const std::vector<uintptr_t> &keys, const std::vector<uintptr_t> &scope)
{
    std::vector<Hold> h;
    for (size_t g = 0; g < keys.size(); ++g) {
        const Hold k{(int32_t)g, 0}, s{(int32_t)g, 1};
        if (scope.empty()) { h.push_back(k); continue; }
        if (keys[g] < scope[g]) { h.push_back(k); h.push_back(s); }
        else { h.push_back(s); h.push_back(k); }
    }
    return h;
}

}  // namespace cper_key
