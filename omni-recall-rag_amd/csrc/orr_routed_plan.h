// orr_routed_plan.h -- the rules of a routed search (orr_search_batch_routed): per query the top `route` documents of a document
// index (normally orr_keys_centroid_index's), then the best chunks of those documents only.
//
//   the twin      per query b the answer is bit for bit what a host composes: (1) orr_search_batch(docs, the query alone,
//                 topk = route, candidate_limit = every row of docs) gives D_b, the routed row ids in rank order; (2)
//                 S_b = orr_scope_create_keys(idx, keys, D_b without kNone), ANDed with `within` if one is given; (3)
//                 orr_search_batch_in_scope(idx, the query alone, topk, candidate_limit, S_b).  An empty S_b gives count 0.
//   arguments     first_invalid: the ORR_EINVAL rules in the order the entry point reports them, before any handle is looked at:
//                 1 an output NULL, 2 route outside 1 .. kMaxRoute, 3 keys NULL, 4 docs NULL; then the search's own.
//   canonical     canonical(D_b): the sorted distinct keys of D_b without kNone -- the set that decides S_b.
//   slots         queries with the same canonical set share one slot (one bitmap, one group of the screening pass); slots are
//                 numbered by first appearance; the empty set is slot kNoSlot: nothing is launched for it, its queries get count 0.
//   slices        at most per_key::kMaxSlots distinct slots each, in slot order; a slice carries the queries of its slots in
//                 ascending query number and, per query, its slot's number inside the slice.
//   union table   per_key::build_table over the slice's sets: key -> the 64-bit mask of the slots that routed to it.
//   keys_include  the sibling of keys_exclude with the opposite rule: include_bits(base, in) -- slot s's 64 bits of a wave are
//                 the base's AND the ballot of (mask >> s) & 1.  A workgroup none of whose rows is routed stores zeros and does
//                 not read the base.
//
// Out of scope: a cluster form, the service mirror and the micro-batcher, a record (shard) form, caller-supplied document content
// built on the device, keeping a document index in step with its source, combining with the diverse or the per-key search, a
// public call that makes many key scopes at once.
//
// Host-only C++17 except the inline marked ORR_PK_HD, which the kernel shares (orr_kernels.hip: keys_include);
// host/orr_routed_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "orr_per_key_plan.h"

namespace routed {

constexpr int64_t kNone = per_key::kNone;
constexpr int32_t kMaxRoute = 1024;
constexpr int32_t kNoSlot = -1;
static_assert((int64_t)per_key::kMaxSlots * kMaxRoute == per_key::kMaxScopeKeys,
              "a slice's union table holds at most as many keys as orr_scope_create_keys takes");

inline bool route_valid(int32_t route) { return route >= 1 && route <= kMaxRoute; }

// The first rule the arguments break, 1 .. 4 in the order the entry point reports them, or 0.
inline int32_t first_invalid(bool out_null, int32_t route, bool keys_null, bool docs_null)
{
    if (out_null) return 1;
    if (!route_valid(route)) return 2;
    if (keys_null) return 3;
    if (docs_null) return 4;
    return 0;
}

// Slot s's 64 bits of a wave: the base's rows whose key the slot routed to.
ORR_PK_HD inline uint64_t include_bits(uint64_t base, uint64_t in) { return base & in; }

// The sorted distinct keys of d[0 .. n) without kNone.
inline std::set<int64_t> canonical(const int64_t *d, int32_t n)
{
    std::set<int64_t> s;
    for (int32_t i = 0; i < n; ++i)
        if (d[i] != kNone) s.insert(d[i]);
    return s;
}

struct Slots {
    std::vector<std::set<int64_t>> sets;               // [n_slots], by first appearance, none empty
    std::vector<int32_t> slot_of;                      // [B]: the query's slot, or kNoSlot
};

// route_keys: [B][route], route_n: [B] (the first route_n[b] entries of a row count).
inline Slots slots(int32_t B, int32_t route, const int64_t *route_keys, const int32_t *route_n)
{
    Slots out;
    out.slot_of.assign((size_t)B, kNoSlot);
    std::map<std::set<int64_t>, int32_t> seen;
    for (int32_t b = 0; b < B; ++b) {
        const int32_t n = route_n[b] < route ? (route_n[b] > 0 ? route_n[b] : 0) : route;
        std::set<int64_t> c = canonical(route_keys + (size_t)b * (size_t)route, n);
        if (c.empty()) continue;
        const auto it = seen.find(c);
        if (it != seen.end()) { out.slot_of[(size_t)b] = it->second; continue; }
        const int32_t s = (int32_t)out.sets.size();
        seen.emplace(c, s);
        out.sets.push_back(std::move(c));
        out.slot_of[(size_t)b] = s;
    }
    return out;
}

struct Slice {
    int32_t slot0, n_slots;                            // slots [slot0, slot0 + n_slots)
    std::vector<int32_t> queries;                      // ascending
    std::vector<int32_t> query_slot;                   // [queries.size()]: the query's slot - slot0
};

inline std::vector<Slice> slices(const Slots &sl)
{
    std::vector<Slice> out;
    const int32_t n = (int32_t)sl.sets.size();
    for (int32_t s0 = 0; s0 < n; s0 += per_key::kMaxSlots) {
        Slice c{s0, std::min<int32_t>(per_key::kMaxSlots, n - s0), {}, {}};
        for (int32_t b = 0; b < (int32_t)sl.slot_of.size(); ++b) {
            const int32_t s = sl.slot_of[(size_t)b];
            if (s < s0 || s >= s0 + c.n_slots) continue;
            c.queries.push_back(b);
            c.query_slot.push_back(s - s0);
        }
        out.push_back(std::move(c));
    }
    return out;
}

// The union table of a slice: per_key::build_table over its slots' sets.
inline void slice_table(const Slots &sl, const Slice &c, std::vector<int64_t> &keys, std::vector<uint64_t> &masks)
{
    std::vector<const std::set<int64_t> *> sets((size_t)c.n_slots);
    for (int32_t i = 0; i < c.n_slots; ++i) sets[(size_t)i] = &sl.sets[(size_t)(c.slot0 + i)];
    per_key::build_table(sets, keys, masks);
}

}  // namespace routed
