// orr_cluster_scope_plan.h -- the rules of a scoped or masked search over the shards of a cluster
// (orr_cluster_search_batch_scoped, orr_cluster_search_batch_masked) and of the shard call the masked one drives
// (orr_search_shard_masked).
//
// Every shard resolves the scope for itself (its own id table, its own deleted rows) and reports the live rows it found; the
// rules below say what the host does with those numbers:
//   split     candidate_limit is GLOBAL over the scoped live rows in the global candidate order (shard 0's rows, then shard
//             1's, ...).  Shard g lets its first took_g = min(live_g, max(0, max(1, limit) - before_g)) scoped live rows take
//             part, before_g the scoped live rows of the shards in front (an exclusive prefix sum).  The tooks add up to
//             min(sum of lives, max(1, limit)): exactly the rows ONE index over all rows would let take part.
//   ladder    every shard answers with k' records per query, the merge certifies (orr_merge_candidates_ex).  A query the merge
//             leaves uncertified repeats, alone or with the others of its kind:
//               k' x 4 while that fits a selection list (the shards keep their path: for a masked search the screen where the
//               library chose it);
//               then, masked search only, the same k' on the list path (pass = 1: no screen, no survivors' buffer to overflow);
//               from there k' x 4 again, ending at the largest took of any shard: there every scoped row of every shard is a
//               record, nothing was cut, and the merge certifies by construction.  Still uncertified there: ORR_EDEVICE.
//             k' never decreases and (path, k') grows strictly, so the ladder ends: ladder_bound() steps at the most.
//   slices    the records of one merge, shards x queries x (k' + 1) records of 56 bytes, stay within a budget; a rung whose
//             queries would not fit runs in slices of merge_slice() queries (at least one).
//
// Host-only C++17; host/orr_cluster_scope_plan_selftest.cpp checks all of it against brute-force restatements on a machine
// without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_escalation.h"

namespace cscope {

// ---- the split of the global limit ---------------------------------------------------------------------------------------
// Scoped live rows a shard may still let take part when `before` scoped live rows lie on the shards in front of it.
inline int64_t shard_limit(int64_t candidate_limit, int64_t before)
{
    return std::max<int64_t>(0, std::max<int64_t>(1, candidate_limit) - std::max<int64_t>(0, before));   // Take(Math.Max(1, maxCount))
}
inline int64_t shard_took(int64_t live, int64_t candidate_limit, int64_t before)
{
    return std::min<int64_t>(std::max<int64_t>(0, live), shard_limit(candidate_limit, before));
}

struct Split {
    std::vector<int64_t> before, took;      // [shards]
    int64_t total = 0, largest = 0;         // sum and maximum of took
};
// live[g]: scoped live rows of shard g, in shard order.
inline Split split_limit(const std::vector<int64_t> &live, int64_t candidate_limit)
{
    Split s;
    s.before.resize(live.size());
    s.took.resize(live.size());
    int64_t in_front = 0;
    for (size_t g = 0; g < live.size(); ++g) {
        s.before[g] = in_front;
        s.took[g] = shard_took(live[g], candidate_limit, in_front);
        s.total += s.took[g];
        s.largest = std::max(s.largest, s.took[g]);
        in_front += std::max<int64_t>(0, live[g]);
    }
    return s;
}

// ---- the ladder ------------------------------------------------------------------------------------------------------------
// `pass` is orr_search_shard_masked's argument: 0 the library's choice (the screen where it pays), 1 the list path.  A scoped
// search has the list path only and stays at 0.
struct Rung {
    int64_t kprime = 0;
    int32_t pass = 0;
    bool done = false;      // nothing more exact exists
};

// The first pass: k' as a single index picks it over the rows that take part in all.  A masked search whose k' no selection
// list holds is on the list path from the start (every shard takes it whatever `pass` says).
inline Rung first_rung(bool masked, int32_t take, int64_t total_took, int32_t sel_width)
{
    const int64_t kprime = escalation::initial_kprime(take, total_took, sel_width);
    return Rung{kprime, masked && kprime > sel_width ? 1 : 0, false};
}

// The pass of the queries `cur` left uncertified.  largest: the largest took of any shard (scoped search: and of any such
// query); screened: some shard answered one of them from behind a screen (ORR_CAND_TWO_STAGE in its trailer) -- where none
// did, the pass WAS the list path, and running it again as pass 1 would change nothing.
inline Rung next_rung(const Rung &cur, bool masked, bool screened, int64_t largest, int32_t sel_width)
{
    const int64_t top = std::max<int64_t>(1, largest);
    const bool on_list = !masked || cur.pass == 1 || !screened;
    const int32_t list_pass = masked ? 1 : 0;
    if (on_list && cur.kprime >= top) return Rung{cur.kprime, list_pass, true};          // every scoped row was a record already
    if (!on_list) {                                                                      // behind a screen
        if (cur.kprime * 4 <= sel_width && cur.kprime < top) return Rung{std::min(cur.kprime * 4, top), 0, false};
        return Rung{cur.kprime, 1, false};
    }
    return Rung{cur.kprime > (INT64_MAX >> 2) ? top : std::min(cur.kprime * 4, top), list_pass, false};
}

// Passes a query goes through at the most, the first included: each step but the one that changes the path multiplies k' by 4
// (or ends at `largest`), from k' >= 1.
inline int ladder_bound(int64_t largest)
{
    int steps = 0;
    for (int64_t k = 1; k < std::max<int64_t>(1, largest); k = k > (INT64_MAX >> 2) ? INT64_MAX : k * 4) ++steps;
    return 1 + steps + 1;       // the first pass, the x 4 steps, the change of path
}
constexpr int kMaxRungs = 34;   // ladder_bound(INT64_MAX)

// ---- the slices of a merge -------------------------------------------------------------------------------------------------
constexpr size_t kRecordBytes = 56;
inline int32_t merge_slice(int32_t nq, int32_t shards, int64_t kprime, size_t budget)
{
    const size_t per_query = (size_t)std::max<int32_t>(shards, 1) * ((size_t)std::max<int64_t>(kprime, 1) + 1) * kRecordBytes;
    const size_t fit = std::max<size_t>(1, budget / per_query);
    return (int32_t)std::min<size_t>((size_t)std::max<int32_t>(nq, 1), fit);
}

}  // namespace cscope
