// orr_cluster_diverse_plan.h -- the host plan of the pair step of a diverse search over a cluster's shards
// (orr_cluster_search_batch_diverse, orr_cluster_pair_dots).  The pool, the cosine and the greedy pass are the single index's
// (orr_diverse_plan.h); what the cluster adds is that the two rows of a pair may lie on different shards.  The plan turns the
// pools' order keys into the work that brings them together:
//
//   locate     an order key is (shard, position) by the shards' row_base and row counts.  Empty shards hold no key; a key
//              outside every shard is an error (Plan::ok false), never a guess.
//   home       a list's home shard holds most of its members, a tie going to the lowest shard index (home_of).  Members on the
//              home shard are read where they lie; every other member is FOREIGN and is copied into the home's staging buffer.
//              A list of n members over G shards therefore moves at most foreign_bound(n, G) = n - ceil(n / G) rows, and a
//              list on one shard moves none.
//   gather     each source shard gets the list of its positions to gather into a dense buffer, in the order (home ascending,
//              then list and rank ascending); a row wanted by two lists is gathered twice.
//   staging    home h's staging buffer holds its foreign rows in the order (source ascending, then list and rank ascending):
//              the rows source s sends to home h are ONE run in s's gather buffer and ONE run in h's staging buffer (Run), so
//              the transport is at most G (G - 1) contiguous copies a group.  List::at[i] is slot i's position on the home
//              shard, or its row in the staging buffer where bit i of List::foreign is set.
//   groups     the lists are cut into groups of consecutive lists: a group's staged rows stay within kStageBudgetBytes (a
//              single list that alone exceeds it is a group of its own) and no home compares more than kListsPerLaunch lists,
//              so a group is at most ONE gather launch per source shard and ONE pair-dot launch per home shard.
//   no dots    a query that reads no cosine (diverse::needs_dots) is in no list.
//
// Host-only C++17; host/orr_cluster_diverse_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "orr_diverse_plan.h"

namespace cdiverse {

constexpr int64_t kStageBudgetBytes = 64ll << 20;    // staged rows of one group, all homes together (DESIGN 8t says why)
constexpr int32_t kListsPerLaunch = 1024;            // lists of one home in one group: the single index's launch limit

struct Place {
    int32_t shard;
    int64_t pos;
};

// Shard g holds the order keys base[g] .. base[g] + rows[g] - 1.  false: no shard holds `key`.
inline bool locate(const std::vector<int64_t> &base, const std::vector<int64_t> &rows, int64_t key, Place *out)
{
    for (size_t g = 0; g < base.size(); ++g)
        if (rows[g] > 0 && key >= base[g] && key - base[g] < rows[g]) {
            *out = Place{(int32_t)g, key - base[g]};
            return true;
        }
    return false;
}

// the shard that holds most of the n >= 1 members; a tie goes to the lowest shard index
inline int32_t home_of(const Place *m, int32_t n, int32_t n_shards)
{
    std::vector<int32_t> held((size_t)n_shards, 0);
    for (int32_t i = 0; i < n; ++i) held[(size_t)m[i].shard] += 1;
    int32_t home = 0;
    for (int32_t g = 1; g < n_shards; ++g)
        if (held[(size_t)g] > held[(size_t)home]) home = g;
    return home;
}

// the most rows a list of n members over n_shards shards moves
inline int32_t foreign_bound(int32_t n, int32_t n_shards) { return n - (n + n_shards - 1) / n_shards; }

struct List {
    int32_t query = 0;                              // of the call's batch (orr_cluster_pair_dots: the list's number)
    int32_t home = 0;
    int32_t n = 0;                                  // members, 1 .. diverse::kMaxPool
    uint64_t foreign = 0;                           // bit i: slot i reads the staging buffer
    std::array<uint32_t, diverse::kMaxPool> at{};   // slot i: a position on the home shard, or a row of its staging buffer
};

struct Run {                                        // rows src_at .. src_at + rows - 1 of src's gather buffer are rows
    int32_t src, home;                              // home_at .. of home's staging buffer
    int64_t src_at, home_at, rows;
};

struct Group {
    int32_t first = 0, count = 0;                   // lists first .. first + count - 1 of Plan::lists
    std::vector<std::vector<uint32_t>> gather;      // [shards] the positions source shard g gathers, in its buffer's order
    std::vector<int64_t> staged;                    // [shards] rows of home g's staging buffer
    std::vector<std::vector<int32_t>> lists;        // [shards] the lists home g compares (numbers in Plan::lists), ascending
    std::vector<Run> runs;                          // ascending (src, home), none empty
    int64_t moved = 0;                              // rows staged, all homes
};

struct Plan {
    bool ok = true;                                 // false: bad_key of query bad_query lies outside every shard; nothing else is set
    int32_t bad_query = -1;
    int64_t bad_key = 0;
    int32_t stride = 1;                             // the longest list
    std::vector<List> lists;                        // ascending query
    std::vector<int32_t> list_of;                   // [B] a query's list, or -1: it reads no cosine
    std::vector<Group> groups;
    int64_t moved = 0;                              // rows staged over the whole call
};

// keys[b * key_stride + i], i < cnt[b]: the order keys of query b's pool in rank order; needs[b]: whether it reads a cosine.
// dim: floats of a row (what a staged row costs).
inline Plan make_plan(const std::vector<int64_t> &base, const std::vector<int64_t> &rows, int32_t B, int32_t key_stride, const int64_t *keys,
                      const int32_t *cnt, const uint8_t *needs, int32_t dim, int64_t budget_bytes = kStageBudgetBytes,
                      int32_t lists_per_launch = kListsPerLaunch)
{
    const int32_t G = (int32_t)base.size();
    Plan p;
    p.list_of.assign((size_t)B, -1);
    std::vector<std::array<Place, diverse::kMaxPool>> where;
    for (int32_t b = 0; b < B; ++b) {
        if (!needs[b] || cnt[b] < 1) continue;
        List l;
        l.query = b;
        l.n = cnt[b] < diverse::kMaxPool ? cnt[b] : diverse::kMaxPool;
        std::array<Place, diverse::kMaxPool> m{};
        for (int32_t i = 0; i < l.n; ++i) {
            const int64_t key = keys[(size_t)b * (size_t)key_stride + (size_t)i];
            if (!locate(base, rows, key, &m[(size_t)i])) {
                Plan bad;
                bad.ok = false; bad.bad_query = b; bad.bad_key = key;
                return bad;
            }
        }
        l.home = home_of(m.data(), l.n, G);
        for (int32_t i = 0; i < l.n; ++i)
            if (m[(size_t)i].shard != l.home) l.foreign |= 1ull << i;
        if (l.n > p.stride) p.stride = l.n;
        p.list_of[(size_t)b] = (int32_t)p.lists.size();
        p.lists.push_back(l);
        where.push_back(m);
    }
    const int64_t row_bytes = 4 * (int64_t)(dim > 0 ? dim : 0);
    auto foreign_rows = [](const List &l) { int64_t f = 0; for (int32_t i = 0; i < l.n; ++i) f += (l.foreign >> i) & 1; return f; };
    const int32_t n_lists = (int32_t)p.lists.size();
    int32_t l0 = 0;
    while (l0 < n_lists) {
        // ---- the group's extent: at least one list
        std::vector<int32_t> per_home((size_t)G, 0);
        int64_t moved = 0;
        int32_t l1 = l0;
        while (l1 < n_lists) {
            const List &l = p.lists[(size_t)l1];
            const int64_t f = foreign_rows(l);
            if (l1 > l0 && ((moved + f) * row_bytes > budget_bytes || per_home[(size_t)l.home] >= lists_per_launch)) break;
            moved += f;
            per_home[(size_t)l.home] += 1;
            ++l1;
        }
        // ---- its runs: source s sends sent[s][h] rows to home h
        Group g;
        g.first = l0; g.count = l1 - l0; g.moved = moved;
        g.gather.assign((size_t)G, {});
        g.staged.assign((size_t)G, 0);
        g.lists.assign((size_t)G, {});
        std::vector<int64_t> sent((size_t)G * (size_t)G, 0), src_at((size_t)G * (size_t)G, 0), home_at((size_t)G * (size_t)G, 0);
        for (int32_t l = l0; l < l1; ++l) {
            const List &li = p.lists[(size_t)l];
            g.lists[(size_t)li.home].push_back(l);
            for (int32_t i = 0; i < li.n; ++i)
                if ((li.foreign >> i) & 1) sent[(size_t)where[(size_t)l][(size_t)i].shard * (size_t)G + (size_t)li.home] += 1;
        }
        for (int32_t s = 0; s < G; ++s) {
            int64_t at = 0;
            for (int32_t h = 0; h < G; ++h) { src_at[(size_t)s * G + h] = at; at += sent[(size_t)s * G + h]; }
            g.gather[(size_t)s].assign((size_t)at, 0u);
        }
        for (int32_t h = 0; h < G; ++h) {
            int64_t at = 0;
            for (int32_t s = 0; s < G; ++s) { home_at[(size_t)s * G + h] = at; at += sent[(size_t)s * G + h]; }
            g.staged[(size_t)h] = at;
        }
        for (int32_t s = 0; s < G; ++s)
            for (int32_t h = 0; h < G; ++h)
                if (sent[(size_t)s * G + h] > 0) g.runs.push_back(Run{s, h, src_at[(size_t)s * G + h], home_at[(size_t)s * G + h], sent[(size_t)s * G + h]});
        // ---- every member's slot
        std::vector<int64_t> next((size_t)G * (size_t)G, 0);
        for (int32_t l = l0; l < l1; ++l) {
            List &li = p.lists[(size_t)l];
            for (int32_t i = 0; i < li.n; ++i) {
                const Place &pl = where[(size_t)l][(size_t)i];
                if (!((li.foreign >> i) & 1)) { li.at[(size_t)i] = (uint32_t)pl.pos; continue; }
                const size_t sh = (size_t)pl.shard * (size_t)G + (size_t)li.home;
                const int64_t k = next[sh]++;
                g.gather[(size_t)pl.shard][(size_t)(src_at[sh] + k)] = (uint32_t)pl.pos;
                li.at[(size_t)i] = (uint32_t)(home_at[sh] + k);
            }
        }
        p.moved += moved;
        p.groups.push_back(std::move(g));
        l0 = l1;
    }
    return p;
}

}  // namespace cdiverse
