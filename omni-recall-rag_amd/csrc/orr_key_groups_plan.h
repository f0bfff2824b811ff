// orr_key_groups_plan.h -- the rules of the key groups (orr_keys_groups, orr_keys_centroids, orr_scope_centroid): a key column read
// from the rows to the document -- which keys a set of rows carries and how many rows each, and one vector per key, the mean of
// its rows' fp32 embeddings.
//
//   members       of key K: the live rows r with key[r] == K, inside `within` when a scope is given, in candidate order (position
//                 ascending).  orr_keys_groups counts every member of every key but kNone.
//   participating the members whose stored normB satisfies normB > 0.0: rows without an embedding and zero vectors (norm 0) and
//                 rows whose norm is NaN take no part, rows with an infinite norm do.
//   the sum       the participating members u_0 < u_1 < ... < u_{n-1} are cut into blocks of kBlock = 256 consecutive members
//                 (blocks_of).  Per coordinate d, all in fp64, no FMA, no reassociation:
//                     P_j[d] = (((+0.0 + e[u_{256j}][d]) + e[u_{256j+1}][d]) + ...)        in member order
//                     S[d]   = (((+0.0 + P_0[d]) + P_1[d]) + ...)                          in block order
//                 (sum_blocked: what keys_block_sums and keys_block_fold must reproduce bit for bit).  A sum started at +0.0 is
//                 never -0.0, so +0.0 + P_0 == P_0 bit for bit and a key of one block writes its S directly.
//   the finish    c[d] = (float)(S[d] / (double)n) on the HOST, IEEE division, round to nearest even; n == 0: c[d] = +0.0f and
//                 S[d] = +0.0 (finish).  Infinities and NaN coordinates follow IEEE.
//   arguments     first_invalid_groups / _centroids / _scope_centroid: the ORR_EINVAL rules in the order the entry points report
//                 them, before any handle is looked at.
//   sort key      sort_key: int64 -> uint64, order preserving (the radix sort of orr_keys_groups orders unsigned keys);
//                 key_of_sort inverts it.  orr_keys_centroids sorts by the key's index in the call's sorted table, which is the
//                 same order on fewer bits (table_bits).
//   slices        the fp64 sums of a call are formed in slices of slice_keys(dim, option) keys: kSliceBytes of sums at most,
//                 whatever the call lists ("key_groups_slice": 0 this rule, 1 .. kMaxKeys forces a size).
//
// Out of scope: the cluster forms (built since: orr_cluster_key_groups_plan.h defines the blocked order across shards; a host
// may still ask each shard through orr_cluster_keys_shard, but such per-shard sums are not the single index's bits), a mean of
// unit-normalised rows or a weighted mean, sharded.py, the service mirror and the micro-batcher, keys in the shard file, a search
// that ranks documents by centroid (built since: orr_centroid_index_plan.h makes the centroids of all keys the rows of an
// ordinary index, which every search call then ranks).
//
// Host-only C++17 except the inlines marked ORR_KG_HD, which the kernels share (orr_kernels.hip: keys_pairs, keys_block_sums,
// keys_block_fold, keys_centroid_finish); host/orr_key_groups_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ORR_KG_HD __host__ __device__
#else
#define ORR_KG_HD
#endif

namespace key_groups {

constexpr int32_t kBlock = 256;                      // members of one block of the sum: PART OF THE CONTRACT (the bits depend on it)
constexpr int32_t kMaxKeys = 65536;                  // keys one orr_keys_centroids call lists (== per_key::kMaxScopeKeys)
constexpr int64_t kSliceBytes = (int64_t)64 << 20;   // fp64 sums of one slice under the library's rule
constexpr uint32_t kDirect = 0xFFFFFFFFu;            // Block::part of a key of one block: its partial IS its sum
constexpr int32_t kCoordsPerLane = 4;                // keys_block_sums: a lane owns four consecutive coordinates ...
constexpr int32_t kCoordsPerPass = kBlock * kCoordsPerLane;   // ... per 1,024

// orr_keys_groups: 1 cap negative, 2 out_n or out_total NULL, 3 out_keys or out_rows NULL with cap > 0, 4 the keys handle NULL
inline int32_t first_invalid_groups(int64_t cap, bool out_keys_null, bool out_rows_null, bool out_n_null, bool out_total_null, bool handle_null)
{
    if (cap < 0) return 1;
    if (out_n_null || out_total_null) return 2;
    if (cap > 0 && (out_keys_null || out_rows_null)) return 3;
    if (handle_null) return 4;
    return 0;
}

// orr_keys_centroids: 1 n_keys outside 0 .. kMaxKeys, 2 keys NULL with n_keys > 0, 3 out_used NULL with n_keys > 0, 4 the keys
// handle NULL.  (dim is looked at with the handle: ORR_EDIM.)
inline int32_t first_invalid_centroids(int32_t n_keys, bool keys_null, bool out_used_null, bool handle_null)
{
    if (n_keys < 0 || n_keys > kMaxKeys) return 1;
    if (n_keys > 0 && keys_null) return 2;
    if (n_keys > 0 && out_used_null) return 3;
    if (handle_null) return 4;
    return 0;
}

// orr_scope_centroid: 1 out_used NULL, 2 the scope NULL
inline int32_t first_invalid_scope_centroid(bool out_used_null, bool scope_null)
{
    if (out_used_null) return 1;
    if (scope_null) return 2;
    return 0;
}

// int64 order as uint64 order
ORR_KG_HD inline uint64_t sort_key(int64_t key) { return (uint64_t)key ^ 0x8000000000000000ull; }
ORR_KG_HD inline int64_t key_of_sort(uint64_t s) { return (int64_t)(s ^ 0x8000000000000000ull); }

// whether a row with this stored norm takes part in a sum (false for 0, negative and NaN; true for +inf)
ORR_KG_HD inline bool participates(double norm_b) { return norm_b > 0.0; }

// the bits a radix sort of table indices 0 .. n_table - 1 has to look at (at least 1)
inline int32_t table_bits(int32_t n_table)
{
    int32_t b = 1;
    while (b < 32 && ((int64_t)1 << b) < (int64_t)n_table) ++b;
    return b;
}

// One block of a key's participating members: pairs [first, first + len) of the sorted pair list, 1 <= len <= kBlock; slot: the
// key's row of the slice's sums; index: the block's number in its key; part: its row of the partial sums, kDirect for a key of
// one block (keys_block_sums then writes the slice's sums itself).
struct Block {
    uint32_t first, len, slot, index, part;
};
// A key of several blocks: keys_block_fold adds partial rows part0 .. part0 + n_blocks - 1, in this order, into row `slot`.
struct Fold {
    uint32_t slot, part0, n_blocks;
};

inline int64_t n_blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

// Cuts the run of n members that starts at pair `first` into blocks, appended to `blocks`; a run of several blocks takes the
// next n_blocks_of(n) rows of the partial sums from `next_part` on and appends its Fold.  n == 0 appends nothing.
inline void blocks_of(int64_t n, int64_t first, uint32_t slot, std::vector<Block> &blocks, std::vector<Fold> &folds, uint32_t &next_part)
{
    const int64_t nb = n_blocks_of(n);
    if (nb > 1) folds.push_back(Fold{slot, next_part, (uint32_t)nb});
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t at = b * kBlock, len = n - at < kBlock ? n - at : kBlock;
        blocks.push_back(Block{(uint32_t)(first + at), (uint32_t)len, slot, (uint32_t)b, nb > 1 ? next_part++ : kDirect});
    }
}

inline bool slice_option_valid(int64_t v) { return v >= 0 && v <= kMaxKeys; }

// keys per slice: the option when it is set, else as many as kSliceBytes of fp64 sums hold; 1 .. kMaxKeys
inline int32_t slice_keys(int32_t dim, int64_t option)
{
    if (option >= 1 && option <= kMaxKeys) return (int32_t)option;
    const int64_t per_key = (int64_t)sizeof(double) * (dim > 0 ? dim : 1);
    const int64_t k = kSliceBytes / per_key;
    return (int32_t)(k < 1 ? 1 : k > kMaxKeys ? kMaxKeys : k);
}

// The rule: S[0 .. dim) of the n rows emb[member[i] * dim ..], i ascending.  volatile keeps a host compiler from contracting or
// reordering the adds whatever its flags.
inline void sum_blocked(const float *emb, int32_t dim, const int64_t *member, int64_t n, double *S)
{
    for (int32_t d = 0; d < dim; ++d) {
        volatile double s = +0.0;
        for (int64_t b0 = 0; b0 < n; b0 += kBlock) {
            volatile double p = +0.0;
            const int64_t b1 = b0 + kBlock < n ? b0 + kBlock : n;
            for (int64_t i = b0; i < b1; ++i) p = p + (double)emb[(size_t)member[i] * (size_t)dim + (size_t)d];
            s = s + p;
        }
        S[d] = s;
    }
}

// One coordinate of the finish, n > 0: IEEE fp64 division, then round to nearest even.  The ONE definition: the host's finish
// and the device's (keys_centroid_finish) both call it.
ORR_KG_HD inline float finish_one(double S, int64_t n) { return (float)(S / (double)n); }

// The finish: c = (float)(S / n), n == 0: +0.0f (and S is +0.0 then: sum_blocked of no rows)
inline void finish(const double *S, int64_t n, int32_t dim, float *c)
{
    for (int32_t d = 0; d < dim; ++d) c[d] = n > 0 ? finish_one(S[d], n) : +0.0f;
}

}  // namespace key_groups
