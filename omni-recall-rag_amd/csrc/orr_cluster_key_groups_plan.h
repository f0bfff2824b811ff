// orr_cluster_key_groups_plan.h -- what a cluster adds to the key groups (orr_cluster_keys_groups, orr_cluster_keys_centroids,
// orr_cluster_scope_centroid).  The contract: the answers of the single-index call on ONE index holding all the cluster's rows in
// the global candidate order (shard 0's rows, then shard 1's, ...), bit for bit.  The single-index rule (orr_key_groups_plan.h)
// stays as it is; this header says how its blocked order runs ACROSS shards.
//
//   members    of key K on a cluster: shard 0's participating members in position order, then shard 1's, ...  For shard g,
//              count = K's participating members on the shard, before = their number on the shards in front, total = the sum of
//              the counts.  Blocks of kBlock = 256 are counted from the key's first member anywhere, so a block may straddle a
//              border (cut):
//   head       before % 256 != 0: the first min(count, 256 - before % 256) members continue the block left open in front of this
//              shard; their running sum starts from that block's carry P, not from +0.0.
//   free       the members behind the head are cut into blocks of 256 from +0.0: exactly keys_block_sums' blocks.
//   closing    a block closes on the shard where its 256th member lies, or the key's last member.  Closed blocks are added to the
//              running S in block order; S starts at +0.0 on the key's first shard and otherwise continues from the S the shard in
//              front left.  A block still open at the end of a shard ((before + count) % 256 != 0 and members follow) is not
//              folded: its partial sum is the carry P for the next shard that holds a member.
//   records    records_of: per shard and slice, key_groups::Block / Fold records for the two existing kernels (a key wholly on the
//              shard gets exactly key_groups::blocks_of's records; a spanning key gets Blocks for its free blocks, each with a
//              partial row, never kDirect) and one Chain record per spanning key with members here, for keys_chain_step.
//   state      per spanning key two rows of dim fp64: S (row 2 * state) and P (row 2 * state + 1).  It travels from shard to shard
//              in ascending order; a shard without a member of the key is skipped, the carry passes over it.
//   execution  run_records: a host executor of one shard's records, add for add what the three kernels are specified to do, so
//              that plan plus execution can be held against key_groups::sum_blocked over the concatenated members without a GPU.
//   groups     merge_groups: the shards' ascending (key, rows) lists merged into one, the rows of equal keys added.
//   arguments  first_invalid_*: the ORR_EINVAL rules of the three entry points, those of key_groups, for the cluster handles.
//
// fp64 addition is not associative: "blocks restart at the border" and "per-shard blocked sums added up" differ from the single
// index's bits whenever a cut is not on a block edge.
//
// Host-only C++17 except the inlines marked ORR_KG_HD, which keys_chain_step shares (orr_kernels.hip);
// host/orr_cluster_key_groups_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_key_groups_plan.h"

namespace cluster_key_groups {

using key_groups::kBlock;

// The argument rules and their order are the single index's (the handle is the cluster's).
inline int32_t first_invalid_groups(int64_t cap, bool out_keys_null, bool out_rows_null, bool out_n_null, bool out_total_null, bool handle_null)
{
    return key_groups::first_invalid_groups(cap, out_keys_null, out_rows_null, out_n_null, out_total_null, handle_null);
}
inline int32_t first_invalid_centroids(int32_t n_keys, bool keys_null, bool out_used_null, bool handle_null)
{
    return key_groups::first_invalid_centroids(n_keys, keys_null, out_used_null, handle_null);
}
inline int32_t first_invalid_scope_centroid(bool out_used_null, bool scope_null)
{
    return key_groups::first_invalid_scope_centroid(out_used_null, scope_null);
}

// The shards' ascending (key, rows) lists as ONE ascending list, the rows of equal keys added.  Returns the number of distinct
// keys; out_keys / out_rows hold the first min(cap, total) entries.
inline int64_t merge_groups(const std::vector<std::vector<int64_t>> &keys, const std::vector<std::vector<int64_t>> &rows, int64_t cap,
                            std::vector<int64_t> &out_keys, std::vector<int64_t> &out_rows)
{
    out_keys.clear(); out_rows.clear();
    std::vector<size_t> at(keys.size(), 0);
    int64_t total = 0;
    for (;;) {
        bool any = false;
        int64_t lowest = 0;
        for (size_t g = 0; g < keys.size(); ++g)
            if (at[g] < keys[g].size() && (!any || keys[g][at[g]] < lowest)) { lowest = keys[g][at[g]]; any = true; }
        if (!any) break;
        int64_t n = 0;
        for (size_t g = 0; g < keys.size(); ++g)
            while (at[g] < keys[g].size() && keys[g][at[g]] == lowest) n += rows[g][at[g]++];
        if (total < cap) { out_keys.push_back(lowest); out_rows.push_back(n); }
        ++total;
    }
    return total;
}

enum : uint32_t { kOpenNone = 0, kOpenHead = 1, kOpenFree = 2 };

// One shard's share of a key: see the file comment.  count == 0: everything zero, the shard is skipped.
struct Cut {
    int32_t head = 0;             // members of the head fragment, 0 .. 255
    int64_t n_free = 0;           // free blocks (from +0.0) on this shard
    int64_t n_close = 0;          // ... of them those that close here: all, or all but the last
    bool head_closes = false;     // the head's block closes here: S = S + P
    uint32_t open = kOpenNone;    // the block left open for the next shard: none, the head's, the last free block
    bool seed_s = false;          // S continues from the shard in front (before > 0)
    bool seed_p = false;          // the head continues an open block: P starts from the carry
};

inline Cut cut(int64_t before, int64_t count, int64_t total)
{
    Cut c;
    if (count <= 0) return c;
    const int64_t in_open = before % kBlock;
    if (in_open != 0) c.head = (int32_t)(count < kBlock - in_open ? count : kBlock - in_open);
    const int64_t rest = count - c.head, end = before + count;
    c.n_free = key_groups::n_blocks_of(rest);
    const bool stays_open = end % kBlock != 0 && end < total;
    c.open = !stays_open ? kOpenNone : rest > 0 ? kOpenFree : kOpenHead;
    c.n_close = c.open == kOpenFree ? c.n_free - 1 : c.n_free;
    c.head_closes = c.head > 0 && c.open != kOpenHead;
    c.seed_s = before > 0;
    c.seed_p = c.head > 0;
    return c;
}

// whether a key with `count` members on a shard of `total` anywhere spans shards (and takes part in the chain on this shard)
inline bool spans(int64_t count, int64_t total) { return count > 0 && count < total; }

// One spanning key's step on one shard (keys_chain_step).  Per coordinate, all fp64, in this order:
//   P = seed_p ? state P row : +0.0;  P = P + e over pairs [head_first, head_first + head_len) in order
//   S = seed_s ? state S row : +0.0;  head closes: S = S + P
//   S = S + parts row (part0 + j), j = 0 .. n_close - 1
//   state S row = S;  open == kOpenHead: state P row = P;  open == kOpenFree: state P row = parts row (part0 + n_close)
struct Chain {
    uint32_t state, head_first, head_len, part0, n_close, flags;
};
enum : uint32_t { kSeedS = 1u, kSeedP = 2u, kHeadCloses = 4u, kOpenShift = 3 };
ORR_KG_HD inline bool chain_seed_s(uint32_t flags) { return (flags & kSeedS) != 0; }
ORR_KG_HD inline bool chain_seed_p(uint32_t flags) { return (flags & kSeedP) != 0; }
ORR_KG_HD inline bool chain_head_closes(uint32_t flags) { return (flags & kHeadCloses) != 0; }
ORR_KG_HD inline uint32_t chain_open(uint32_t flags) { return (flags >> kOpenShift) & 3u; }

struct Records {
    std::vector<key_groups::Block> blocks;
    std::vector<key_groups::Fold> folds;
    std::vector<Chain> chains;
    uint32_t n_parts = 0;
    void clear() { blocks.clear(); folds.clear(); chains.clear(); n_parts = 0; }
};

// One shard's records of a slice of ns keys: count / first (the key's run in this shard's sorted pair list), before and total per
// key; state[j] is the key's state slot where it spans shards (any shard holds some but not all of its members), ignored
// otherwise; slot[j] (NULL: j) is the row of this shard's sums a key wholly here is summed into -- a shard keeps rows for its own
// keys only, so that the slice's sums come to the host once, not once per shard.
inline void records_of(int32_t ns, const int64_t *count, const int64_t *first, const int64_t *before, const int64_t *total, const int32_t *state,
                       const int32_t *slot, Records &r)
{
    for (int32_t j = 0; j < ns; ++j) {
        if (count[j] <= 0) continue;
        if (!spans(count[j], total[j])) {               // wholly here: the single index's path and records
            key_groups::blocks_of(count[j], first[j], (uint32_t)(slot ? slot[j] : j), r.blocks, r.folds, r.n_parts);
            continue;
        }
        const Cut c = cut(before[j], count[j], total[j]);
        const int64_t rest = count[j] - c.head, block0 = (before[j] + c.head) / kBlock;
        Chain ch{(uint32_t)state[j], (uint32_t)first[j], (uint32_t)c.head, r.n_parts, (uint32_t)c.n_close,
                 (c.seed_s ? kSeedS : 0u) | (c.seed_p ? kSeedP : 0u) | (c.head_closes ? kHeadCloses : 0u) | (c.open << kOpenShift)};
        for (int64_t b = 0; b < c.n_free; ++b) {
            const int64_t at = b * kBlock, len = rest - at < kBlock ? rest - at : kBlock;
            r.blocks.push_back(key_groups::Block{(uint32_t)(first[j] + c.head + at), (uint32_t)len, (uint32_t)j, (uint32_t)(block0 + b), r.n_parts++});
        }
        r.chains.push_back(ch);
    }
}

// One shard's records applied on the host exactly as keys_block_sums, keys_block_fold and keys_chain_step are specified to:
// emb [.][dim], pos the shard's sorted pair positions, sums [slots][dim], parts [n_parts][dim], state [spanning keys][2][dim].
// volatile keeps a host compiler from contracting or reordering the adds whatever its flags.
inline void run_records(const Records &r, const float *emb, int32_t dim, const uint32_t *pos, double *sums, double *parts, double *state)
{
    const size_t D = (size_t)dim;
    for (const key_groups::Block &b : r.blocks) {
        double *out = b.part == key_groups::kDirect ? sums + (size_t)b.slot * D : parts + (size_t)b.part * D;
        for (size_t d = 0; d < D; ++d) {
            volatile double p = +0.0;
            for (uint32_t i = 0; i < b.len; ++i) p = p + (double)emb[(size_t)pos[(size_t)b.first + i] * D + d];
            out[d] = p;
        }
    }
    for (const key_groups::Fold &f : r.folds)
        for (size_t d = 0; d < D; ++d) {
            volatile double s = +0.0;
            for (uint32_t b = 0; b < f.n_blocks; ++b) s = s + parts[((size_t)f.part0 + b) * D + d];
            sums[(size_t)f.slot * D + d] = s;
        }
    for (const Chain &c : r.chains) {
        double *S = state + (size_t)c.state * 2 * D, *P = S + D;
        for (size_t d = 0; d < D; ++d) {
            volatile double p = chain_seed_p(c.flags) ? P[d] : +0.0;
            for (uint32_t i = 0; i < c.head_len; ++i) p = p + (double)emb[(size_t)pos[(size_t)c.head_first + i] * D + d];
            volatile double s = chain_seed_s(c.flags) ? S[d] : +0.0;
            if (chain_head_closes(c.flags)) s = s + p;
            for (uint32_t j = 0; j < c.n_close; ++j) s = s + parts[((size_t)c.part0 + j) * D + d];
            S[d] = s;
            if (chain_open(c.flags) == kOpenHead) P[d] = p;
            else if (chain_open(c.flags) == kOpenFree) P[d] = parts[((size_t)c.part0 + c.n_close) * D + d];
        }
    }
}

}  // namespace cluster_key_groups
