// orr_centroid_index_plan.h -- the rules of the document index (orr_keys_centroid_index) and of the read-back of stored rows
// (orr_index_get_rows): a sealed orr_index whose rows are the centroids of ALL keys of a key column, built on the device.
//
//   the twin      the result answers every call bit for bit like the index a host builds from orr_keys_groups (all distinct keys,
//                 ascending) and orr_keys_centroids (the float centroids and out_used): the keys with out_used == 0 dropped, one
//                 row per kept key in ascending key order -- embedding the centroid (key_groups::finish_one: the ONE expression
//                 host and device share), created_ticks those of the key's first participating member in candidate order,
//                 row_id the key, content empty -- appended to a fresh index of the source's device and dim, then sealed.
//   arguments     first_invalid: the ORR_EINVAL rules in the order the entry point reports them, before any handle is looked
//                 at; first_invalid_get_rows likewise.
//   all keys      the distinct keys of the members (orr_keys_groups' list, as key_groups::sort_key values, ascending) and the
//                 runs of the PARTICIPATING members sorted by the same key (a subset, ascending): merge_runs gives each key its
//                 participating count (0: no run) and the pair where its run starts.
//   kept          kept(used): a key is kept when at least one member participates; the others are skipped and counted.
//   slices        the keys are walked in slices of key_groups::slice_keys keys of the ALL-keys list (walk); a key's row of the
//                 slice's fp64 sums is its number in the slice, kept or not (Kept::slot); the kept keys of a slice are written
//                 densely, in key order (slice_kept), and land at rows Slice::row0 .. row0 + n_kept - 1 of the result.  A
//                 slice without a kept key launches nothing and appends nothing.
//   get_rows      rows per slice of the gather's workspace (get_rows_slice): kGatherBytes at most, one row at least.
//
// Out of scope: a cluster form (the host route over orr_cluster_keys_centroids remains), caller-supplied content per document, a
// routed two-level call, keeping the derived index in step with the source, sharded.py, the service mirror and the
// micro-batcher, keys in the shard file, a pinned return path for orr_keys_centroids.
//
// Host-only C++17 (the kernels read Kept; the finish expression is orr_key_groups_plan.h's);
// host/orr_centroid_index_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_key_groups_plan.h"

namespace centroid_index {

constexpr int64_t kGatherBytes = (int64_t)64 << 20;   // fp32 rows one slice of orr_index_get_rows gathers

// orr_keys_centroid_index: 1 out NULL, 2 the keys handle NULL
inline int32_t first_invalid(bool out_null, bool handle_null)
{
    if (out_null) return 1;
    if (handle_null) return 2;
    return 0;
}

// orr_index_get_rows: 1 n negative, 2 row_ids or out_emb NULL with n > 0, 3 the index NULL.  (dim is looked at with the handle.)
inline int32_t first_invalid_get_rows(int64_t n, bool ids_null, bool out_null, bool handle_null)
{
    if (n < 0) return 1;
    if (n > 0 && (ids_null || out_null)) return 2;
    if (handle_null) return 3;
    return 0;
}

inline bool kept(int64_t used) { return used > 0; }

// A kept key of a slice, as keys_centroid_finish reads it: slot its row of the slice's sums, n its participating members,
// first the pair of its first participating member (the newest chunk that takes part).  Its destination is its index in the
// slice's list.
struct Kept {
    uint32_t slot, n, first;
};

// One slice of the walk: keys [key0, key0 + n_keys) of the ALL-keys list, n_kept of them kept, written to rows row0 .. of the result.
struct Slice {
    int64_t key0;
    int32_t n_keys;
    int64_t row0;
    int32_t n_kept;
};

// used[i] / first[i] for the T keys all[] (ascending, distinct) from the runs rk[] / rl[] (ascending, distinct, every rl > 0) of
// the m participating pairs.  false: a run whose key is not listed, a run of no pair, or runs that do not add up to m.
inline bool merge_runs(const uint64_t *all, int64_t T, const uint64_t *rk, const uint32_t *rl, int64_t runs, int64_t m,
                       std::vector<int64_t> &used, std::vector<int64_t> &first)
{
    used.assign((size_t)T, 0);
    first.assign((size_t)T, 0);
    int64_t at = 0, i = 0;
    for (int64_t r = 0; r < runs; ++r) {
        while (i < T && all[i] < rk[r]) ++i;
        if (i >= T || all[i] != rk[r] || rl[r] == 0 || at + (int64_t)rl[r] > m) return false;
        used[(size_t)i] = (int64_t)rl[r];
        first[(size_t)i] = at;
        at += (int64_t)rl[r];
        ++i;
    }
    return at == m;
}

// The kept keys of slice [s0, s0 + ns), in key order, appended to `out`; their number.
inline int32_t slice_kept(const int64_t *used, const int64_t *first, int64_t s0, int32_t ns, std::vector<Kept> &out)
{
    int32_t n = 0;
    for (int32_t j = 0; j < ns; ++j)
        if (kept(used[s0 + j])) {
            out.push_back(Kept{(uint32_t)j, (uint32_t)used[s0 + j], (uint32_t)first[s0 + j]});
            ++n;
        }
    return n;
}

// The walk over T keys in slices of per_slice (>= 1): every slice, the empty ones included (n_kept == 0: nothing is launched).
inline std::vector<Slice> walk(const int64_t *used, int64_t T, int32_t per_slice)
{
    std::vector<Slice> out;
    int64_t row = 0;
    for (int64_t s0 = 0; s0 < T; s0 += per_slice) {
        const int32_t ns = (int32_t)(T - s0 < (int64_t)per_slice ? T - s0 : (int64_t)per_slice);
        int32_t n = 0;
        for (int32_t j = 0; j < ns; ++j) n += kept(used[s0 + j]) ? 1 : 0;
        out.push_back(Slice{s0, ns, row, n});
        row += n;
    }
    return out;
}

// rows of dim floats per slice of orr_index_get_rows
inline int64_t get_rows_slice(int32_t dim)
{
    const int64_t per_row = (int64_t)sizeof(float) * (dim > 0 ? dim : 1);
    const int64_t r = kGatherBytes / per_row;
    return r < 1 ? 1 : r;
}

}  // namespace centroid_index
