// orr_per_key_plan.h -- the rules of a per-key search (orr_search_batch_per_key): the plain search's ranking of a query, walked
// from the top, keeping at most max_per_key rows of each key (orr_keys: one int64 per row, typically a document number).
//
//   answer        R = the complete ranking of the call's candidates (orr_search_batch, or orr_search_batch_in_scope with a scope,
//                 for topk = all rows).  Walk R from the top: a row is kept when its key is kNone or fewer than max_per_key kept
//                 rows carry its key; stop at take = max(1, topk) kept (walk_all).  Unlike the diverse search the call DOES look
//                 outside the pool: fewer than take rows come back only when the candidates ran out.
//   arguments     first_invalid: the rules in the order the entry point reports them: 1 an output NULL, 2 pool outside
//                 1 .. kMaxPool, 3 max(1, topk) > pool, 4 max_per_key < 1, 5 keys NULL; then the NULL index, then the search's own.
//   rounds        per query the state is the kept list, a count per key, the closed keys K, the seen positions S, finished.
//                 Round 1 sees the first `pool` rows of R (the call the diverse search makes for its pool).  Round r > 1 sees the
//                 first `pool` rows of the ranking of the FROZEN candidate set C (the rows of round 1: the first
//                 min(live, max(1, candidate_limit)) live rows, of the scope if any) without the rows whose key is in K and
//                 without the positions in S, with no further limit.  walk_round walks a round's rows in order: a row with no key
//                 or a key below its cap is kept; a key reaching max_per_key enters K; any other row is skipped (a key closed
//                 earlier in the same round); the walk ends, and the query is finished, at take kept.  Then every row of the round
//                 enters S.  A round that returned fewer than pool rows finishes the query.  Every round keeps at least one row:
//                 rounds <= take.
//   union table   per slice of at most kMaxSlots unfinished queries: the sorted union of the slots' closed keys, each entry with
//                 the 64-bit mask of the slots that closed it (build_table).  kNone is never listed, and table_mask passes over it
//                 even if it were.
//   lookup        table_find: ONE binary search per row; table_mask: the slots that closed the row's key.
//   keys_exclude  one lane per row, 64 rows a wave = two bitmap words.  exclude_bits(base, closed): slot s's 64 bits are the base's
//                 AND NOT the ballot of (mask >> s) & 1.  A workgroup owns kBlockRows rows = kBlockWords words of every slot and
//                 stores them as 16-byte vectors, 256 contiguous bytes per slot; a workgroup none of whose rows is closed copies
//                 the base words.  The table sits in LDS up to kLdsTable entries (32 KB) and in global memory beyond.
//
// Out of scope: the cluster forms (built since: orr_cluster_per_key_plan.h), the record (shard) form, the service mirror and the
// micro-batcher, keys in the shard file, pools above kMaxPool, combining with the diverse search.
//
// Host-only C++17 except the inlines marked ORR_PK_HD, which the kernels share (orr_kernels.hip: keys_exclude, keys_member);
// host/orr_per_key_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <map>
#include <set>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define ORR_PK_HD __host__ __device__
#else
#define ORR_PK_HD
#endif

namespace per_key {

constexpr int64_t kNone = INT64_MIN;                 // ORR_KEY_NONE
constexpr int32_t kSelWidth = 64;                    // == orr::kSelWidth (orr_api.hip asserts it)
constexpr int32_t kMaxPool = kSelWidth - 8;          // 56, as the diverse search's
constexpr int32_t kMaxSlots = 64;                    // queries of one slice: one bit each of a table entry's mask
constexpr int32_t kMaxScopeKeys = 65536;             // orr_scope_create_keys
constexpr int32_t kLdsTable = 2048;                  // entries (8-byte key + 8-byte mask) the kernels keep in LDS; beyond: global
constexpr int32_t kBlockThreads = 256;
constexpr int32_t kBlockWords = 64;                  // bitmap words of every slot one workgroup of keys_exclude owns
constexpr int32_t kBlockRows = kBlockWords * 32;     // 2048 = 8 rows per thread

inline bool pool_valid(int32_t pool) { return pool >= 1 && pool <= kMaxPool; }
inline int32_t take_of(int32_t topk) { return topk > 1 ? topk : 1; }
ORR_PK_HD inline bool table_in_lds(int32_t n_table) { return n_table <= kLdsTable; }

// The first rule the arguments break, 1 .. 5 in the order the entry point reports them, or 0.
inline int32_t first_invalid(bool out_null, int32_t topk, int32_t pool, int32_t max_per_key, bool keys_null)
{
    if (out_null) return 1;
    if (!pool_valid(pool)) return 2;
    if (take_of(topk) > pool) return 3;
    if (max_per_key < 1) return 4;
    if (keys_null) return 5;
    return 0;
}

// orr_scope_create_keys: 1 out NULL, 2 n_keys outside 0 .. kMaxScopeKeys, 3 keys NULL with n_keys > 0, 4 the keys handle NULL
inline int32_t first_invalid_scope_keys(bool out_null, int32_t n_keys, bool keys_null, bool handle_null)
{
    if (out_null) return 1;
    if (n_keys < 0 || n_keys > kMaxScopeKeys) return 2;
    if (n_keys > 0 && keys_null) return 3;
    if (handle_null) return 4;
    return 0;
}

// ---- the table and its lookup --------------------------------------------------------------------------------------------------
// Index of `key` in keys[0 .. n) (ascending, distinct), or -1: one binary search.
ORR_PK_HD inline int32_t table_find(const int64_t *keys, int32_t n, int64_t key)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < n && keys[lo] == key) ? lo : -1;
}

// The slots that closed `key`: 0 for kNone (never closed, even if listed) and for a key the table does not hold.
ORR_PK_HD inline uint64_t table_mask(const int64_t *keys, const uint64_t *masks, int32_t n, int64_t key)
{
    if (key == kNone) return 0ull;
    const int32_t i = table_find(keys, n, key);
    return i < 0 ? 0ull : masks[i];
}

// Slot s's 64 bits of a wave: the base's, without the rows whose key the slot has closed.
ORR_PK_HD inline uint64_t exclude_bits(uint64_t base, uint64_t closed) { return base & ~closed; }
ORR_PK_HD inline bool slot_closed(uint64_t mask, int32_t slot) { return ((mask >> slot) & 1ull) != 0ull; }

// The sorted union of the slots' closed keys with the mask of the slots that closed each; closed.size() <= kMaxSlots.
inline void build_table(const std::vector<const std::set<int64_t> *> &closed, std::vector<int64_t> &keys, std::vector<uint64_t> &masks)
{
    std::map<int64_t, uint64_t> u;
    for (size_t s = 0; s < closed.size(); ++s)
        for (int64_t k : *closed[s])
            if (k != kNone) u[k] |= 1ull << s;
    keys.clear(); masks.clear();
    for (const auto &e : u) { keys.push_back(e.first); masks.push_back(e.second); }
}

// A sorted list of distinct keys (orr_scope_create_keys: duplicates count once; kNone may be listed and sorts first).
inline std::vector<int64_t> member_table(const int64_t *keys, int32_t n)
{
    std::vector<int64_t> t(keys, keys + n);
    std::sort(t.begin(), t.end());
    t.erase(std::unique(t.begin(), t.end()), t.end());
    return t;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
struct State {
    std::vector<int32_t> kept;                       // what the caller numbers the kept rows by, in walk order
    std::map<int64_t, int32_t> count;                // kept rows per key (kNone is not counted)
    std::set<int64_t> closed;                        // K
    std::vector<int64_t> seen;                       // S, positions
    int32_t rounds = 0;
    bool finished = false;
};

// One round of n rows (their keys, positions and the caller's numbers, in rank order) for a query that is not finished.
inline void walk_round(State &st, int32_t n, const int64_t *keys, const int64_t *pos, const int32_t *number, int32_t take,
                       int32_t max_per_key, int32_t pool)
{
    st.rounds += 1;
    for (int32_t i = 0; i < n && !st.finished; ++i) {
        const int64_t k = keys[i];
        if (k != kNone) {
            if (st.closed.count(k)) continue;          // closed earlier in this round
            int32_t &c = st.count[k];
            c += 1;
            if (c >= max_per_key) st.closed.insert(k);
        }
        st.kept.push_back(number[i]);
        if ((int32_t)st.kept.size() >= take) st.finished = true;
    }
    for (int32_t i = 0; i < n; ++i) st.seen.push_back(pos[i]);
    if (n < pool) st.finished = true;
}

// The one-walk definition over a complete ranking of n rows: the ranks kept, at most take.
inline std::vector<int32_t> walk_all(int32_t n, const int64_t *keys, int32_t take, int32_t max_per_key)
{
    std::vector<int32_t> kept;
    std::map<int64_t, int32_t> count;
    for (int32_t r = 0; r < n && (int32_t)kept.size() < take; ++r) {
        const int64_t k = keys[r];
        if (k != kNone) {
            int32_t &c = count[k];
            if (c >= max_per_key) continue;
            c += 1;
        }
        kept.push_back(r);
    }
    return kept;
}

}  // namespace per_key
