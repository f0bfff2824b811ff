// orr_insert_plan.h -- the host side of orr_index_insert_rows: where the new rows of a sealed shard go, how far the old rows
// move, and the merged token index.  Plain C++ on plain data (no HIP, no index), so that host/orr_insert_plan_selftest runs it
// on a machine without a GPU.
//
// The shard afterwards is what a seal of (old rows in candidate order, then the new rows in the order given) would make: a
// STABLE CreatedAt-descending order (InMemoryIngestionStore.cs:61).  The old rows are already in that order, so the result is
// a merge in which, at equal ticks, every old row stays in front of every new one and the new rows keep their relative order.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "orr_layout.h"
#include "orr_token_index.h"

namespace orr {

struct InsertPlan {
    int64_t n_old = 0, n_new = 0;
    std::vector<int64_t> order;        // [n_new] merged rank k of the new rows -> input row (stable by ticks, descending)
    std::vector<int64_t> new_pos;      // [n_new] final position of new row `order[k]`, strictly ascending
    std::vector<uint32_t> shift;       // [n_old + 1] new rows in front of old position p: p moves to p + shift[p]; shift[n_old] = n_new
    int64_t first_moved = 0;           // positions in front of it keep their rows (= new_pos[0]; n_old without new rows)
    int64_t rows() const { return n_old + n_new; }
};

// old_ticks[n_old]: the shard's timestamps in candidate order (descending); new_ticks[n_new] in the order given.
inline InsertPlan make_insert_plan(const int64_t *old_ticks, int64_t n_old, const int64_t *new_ticks, int64_t n_new)
{
    InsertPlan pl;
    pl.n_old = n_old;
    pl.n_new = n_new;
    pl.order.resize((size_t)n_new);
    std::iota(pl.order.begin(), pl.order.end(), (int64_t)0);
    std::stable_sort(pl.order.begin(), pl.order.end(), [new_ticks](int64_t a, int64_t b) { return new_ticks[a] > new_ticks[b]; });
    pl.new_pos.resize((size_t)n_new);
    pl.shift.resize((size_t)n_old + 1);
    int64_t p = 0;
    for (int64_t k = 0; k < n_new; ++k) {
        const int64_t t = new_ticks[pl.order[(size_t)k]];
        while (p < n_old && old_ticks[p] >= t) pl.shift[(size_t)p++] = (uint32_t)k;      // old rows at least as new stay in front
        pl.new_pos[(size_t)k] = p + k;
    }
    while (p <= n_old) pl.shift[(size_t)p++] = (uint32_t)n_new;
    pl.first_moved = n_new > 0 ? pl.new_pos[0] : n_old;
    return pl;
}

// The sources of the destination positions [d0, d1): src[d - d0] >= 0 is an old position, < 0 is new row ~k (merged rank k).
inline void plan_sources(const InsertPlan &pl, int64_t d0, int64_t d1, int64_t *src)
{
    int64_t k = (int64_t)(std::lower_bound(pl.new_pos.begin(), pl.new_pos.end(), d0) - pl.new_pos.begin());
    int64_t p = d0 - k;                                                    // old rows in front of d0
    for (int64_t d = d0; d < d1; ++d) {
        if (k < pl.n_new && pl.new_pos[(size_t)k] == d) src[d - d0] = ~(k++);
        else src[d - d0] = p++;
    }
}

// A shard FILE holds the timestamps as the device has them, and there a deleted row's timestamp is overwritten with 0
// (orr_index_delete_rows).  The plan reads the timestamps as a descending sequence, so a loaded shard's host mirror gets, at
// every deleted position (dead[], ascending), the ticks of the nearest live row in front of it -- of the first live row
// behind it for deleted rows at the very front; all rows deleted: left alone, they are all equal.  Any value between a dead
// row's neighbours serves: deleted rows take no part in a search and do not count towards candidate_limit.
inline void repair_dead_ticks(std::vector<int64_t> &ticks, const std::vector<int64_t> &dead)
{
    if (dead.empty() || dead.size() >= ticks.size()) return;
    size_t lead = 0;                                                         // deleted rows at the very front
    while (lead < dead.size() && dead[lead] == (int64_t)lead) ++lead;
    for (size_t i = lead; i < dead.size(); ++i) ticks[(size_t)dead[i]] = ticks[(size_t)dead[i] - 1];
    for (size_t i = 0; i < lead; ++i) ticks[i] = ticks[lead];
}

// The deleted positions (ascending) where they are afterwards (still ascending: the shift never decreases).
inline std::vector<int64_t> remap_dead(const InsertPlan &pl, const std::vector<int64_t> &dead)
{
    std::vector<int64_t> out(dead.size());
    for (size_t i = 0; i < dead.size(); ++i) out[i] = dead[i] + (int64_t)pl.shift[(size_t)dead[i]];
    return out;
}

// old_any[n_old] / new_any[n_new in the order GIVEN] merged into candidate order (host mirrors: ticks, content lengths)
template <typename T>
inline std::vector<T> merge_rows(const InsertPlan &pl, const T *old_any, const T *new_any)
{
    std::vector<T> out((size_t)pl.rows());
    for (int64_t p = 0; p < pl.n_old; ++p) out[(size_t)(p + pl.shift[(size_t)p])] = old_any[p];
    for (int64_t k = 0; k < pl.n_new; ++k) out[(size_t)pl.new_pos[(size_t)k]] = new_any[pl.order[(size_t)k]];
    return out;
}

inline uint64_t vocab_pool_bytes(const TokenIndexHost &ti)
{
    return ti.vstart.empty() ? 0 : ti.vstart.back() + padded_row_bytes(ti.vlen.back());
}

// The token index of the merged shard.  `old`: the shard's index (old.vpool may carry slack behind the last token); `add`: the
// index build_token_index makes of the NEW rows alone, laid out in merged rank order (its row k is new row order[k], which
// lands on new_pos[k]).  Every old posting is renumbered through the shift table, the new rows' positions are merged into the
// lists of the tokens that exist, and tokens not seen before are appended to the vocabulary with their lists, in the scan
// kernel's layout (16-byte aligned starts, space padding).  One pass over the old postings.
inline void merge_token_index(const TokenIndexHost &old, const TokenIndexHost &add, const InsertPlan &pl, TokenIndexHost &out)
{
    const size_t V_old = old.vstart.size(), V_add = add.vstart.size();
    auto token_of = [](const TokenIndexHost &ti, size_t v) {
        return std::string_view(reinterpret_cast<const char *>(ti.vpool.data() + ti.vstart[v]), ti.vlen[v]);
    };
    // the new rows' vocabulary is the small side: hash it, then walk the old vocabulary once
    std::unordered_map<std::string_view, uint32_t> add_ids;
    add_ids.reserve(V_add * 2 + 1);
    for (size_t v = 0; v < V_add; ++v) add_ids.emplace(token_of(add, v), (uint32_t)v);
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> add_of_old(V_old, kNone);
    std::vector<uint8_t> seen(V_add, 0);
    if (V_add)
        for (size_t v = 0; v < V_old; ++v) {
            auto it = add_ids.find(token_of(old, v));
            if (it != add_ids.end()) { add_of_old[v] = it->second; seen[it->second] = 1; }
        }
    std::vector<uint32_t> unseen;
    for (size_t v = 0; v < V_add; ++v) if (!seen[v]) unseen.push_back((uint32_t)v);
    const size_t V = V_old + unseen.size();

    out.post_off.assign(V + 1, 0);
    out.post_rows.resize(old.post_rows.size() + add.post_rows.size());
    size_t w = 0;
    auto put_new = [&](uint64_t &i) { out.post_rows[w++] = (uint32_t)pl.new_pos[add.post_rows[(size_t)i++]]; };
    for (size_t v = 0; v < V_old; ++v) {
        out.post_off[v] = w;
        const uint32_t a = add_of_old[v];
        uint64_t i = a == kNone ? 0 : add.post_off[a];
        const uint64_t i_end = a == kNone ? 0 : add.post_off[(size_t)a + 1];
        for (uint64_t j = old.post_off[v]; j < old.post_off[v + 1]; ++j) {
            const uint32_t p = old.post_rows[(size_t)j];
            const uint32_t np = p + pl.shift[p];
            while (i < i_end && (uint32_t)pl.new_pos[add.post_rows[(size_t)i]] < np) put_new(i);
            out.post_rows[w++] = np;
        }
        while (i < i_end) put_new(i);
    }
    for (size_t u = 0; u < unseen.size(); ++u) {
        const uint32_t a = unseen[u];
        out.post_off[V_old + u] = w;
        for (uint64_t i = add.post_off[a]; i < add.post_off[(size_t)a + 1];) put_new(i);
    }
    out.post_off[V] = w;

    out.vstart.resize(V);
    out.vlen.resize(V);
    uint64_t cur = vocab_pool_bytes(old);
    std::copy(old.vstart.begin(), old.vstart.end(), out.vstart.begin());
    std::copy(old.vlen.begin(), old.vlen.end(), out.vlen.begin());
    for (size_t u = 0; u < unseen.size(); ++u) {
        out.vstart[V_old + u] = cur;
        out.vlen[V_old + u] = add.vlen[unseen[u]];
        cur += padded_row_bytes(add.vlen[unseen[u]]);
    }
    out.vpool.assign((size_t)cur, 0x20);
    if (V_old) memcpy(out.vpool.data(), old.vpool.data(), (size_t)vocab_pool_bytes(old));
    for (size_t u = 0; u < unseen.size(); ++u)
        memcpy(out.vpool.data() + out.vstart[V_old + u], add.vpool.data() + add.vstart[unseen[u]], add.vlen[unseen[u]]);
}

}  // namespace orr
