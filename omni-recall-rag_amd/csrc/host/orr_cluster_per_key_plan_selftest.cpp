// orr_cluster_per_key_plan_selftest -- the rules a cluster adds to the per-key search (orr_cluster_per_key_plan.h) against
// brute-force restatements, on a machine without a GPU.  tests/test_cluster_per_key_cpu.py runs it.
#include "../orr_cluster_per_key_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <set>
#include <vector>

using namespace cper_key;

static long g_checks = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        ++g_checks;                                                                    \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static std::vector<int64_t> bases_of(const std::vector<int64_t> &rows)
{
    std::vector<int64_t> base(rows.size());
    int64_t at = 0;
    for (size_t g = 0; g < rows.size(); ++g) { base[g] = at; at += rows[g]; }
    return base;
}

// ---- which shard gathers which members ---------------------------------------------------------------------------------------
static void test_gather()
{
    const std::vector<int64_t> rows{5, 0, 3, 0, 0, 7, 0};                  // empty shards in the middle and at the end
    const std::vector<int64_t> base = bases_of(rows);
    // two queries, pool 4: query 0 has 4 members, query 1 has 2 (its other slots hold what an earlier round left)
    const int64_t keys[8] = {4, 5, 0, 14, 8, 7, 99, -1};
    const int32_t cnt[2] = {4, 2};
    const Gather g = gather_plan(base, rows, 2, 4, keys, cnt);
    CHECK(g.ok && g.pos.size() == 7 && g.at.size() == 7);
    CHECK((g.pos[0] == std::vector<int64_t>{4, 0}) && (g.at[0] == std::vector<int32_t>{0, 2}));
    CHECK((g.pos[2] == std::vector<int64_t>{0, 2}) && (g.at[2] == std::vector<int32_t>{1, 5}));       // key 5: the first row behind the border; key 7: the last before the next
    CHECK((g.pos[5] == std::vector<int64_t>{6, 0}) && (g.at[5] == std::vector<int32_t>{3, 4}));       // key 14: the cluster's last row; key 8: the first of shard 5
    for (int32_t e : {1, 3, 4, 6}) CHECK(g.pos[(size_t)e].empty() && g.at[(size_t)e].empty());         // an empty shard gathers nothing
    // every key of the cluster goes to the shard that holds it, at key - base
    std::vector<int64_t> all(15);
    std::iota(all.begin(), all.end(), 0);
    const int32_t n_all[1] = {15};
    const Gather a = gather_plan(base, rows, 1, 15, all.data(), n_all);
    CHECK(a.ok);
    for (size_t s = 0; s < rows.size(); ++s) {
        CHECK((int64_t)a.pos[s].size() == rows[s]);
        for (size_t i = 0; i < a.pos[s].size(); ++i) CHECK(a.pos[s][i] == (int64_t)i && all[(size_t)a.at[s][i]] == base[s] + (int64_t)i);
    }
    // a key outside every shard is refused and says which; slots at or beyond a query's count are not looked at
    const int32_t over[2] = {4, 3};
    const Gather bad = gather_plan(base, rows, 2, 4, keys, over);
    CHECK(!bad.ok && bad.bad_query == 1 && bad.bad_key == 99 && bad.pos.empty() && bad.at.empty());
    const int64_t neg[1] = {-1};
    const int32_t one[1] = {1};
    CHECK(!gather_plan(base, rows, 1, 1, neg, one).ok);
    const int32_t none[2] = {0, 0};
    const Gather empty = gather_plan(base, rows, 2, 4, keys, none);
    CHECK(empty.ok);
    for (const auto &p : empty.pos) CHECK(p.empty());
}

// ---- seen positions at both sides of every border ------------------------------------------------------------------------------
static void test_seen()
{
    const std::vector<int64_t> rows{5, 0, 3, 1, 7};
    const std::vector<int64_t> base = bases_of(rows);
    const int64_t total = 16;
    // slot 0 has seen every order key, slot 1 the two rows at each border, slot 2 nothing, slot 3 keys outside the cluster
    std::vector<int64_t> s0((size_t)total), s1, s2, s3{-1, total, INT64_MAX, INT64_MIN};
    std::iota(s0.begin(), s0.end(), 0);
    for (size_t g = 1; g < rows.size(); ++g) { s1.push_back(base[g] - 1); s1.push_back(base[g]); }
    const std::vector<const std::vector<int64_t> *> seen{&s0, &s1, &s2, &s3};
    int64_t got0 = 0;
    for (size_t g = 0; g < rows.size(); ++g) {
        const Seen s = seen_of_shard(base[g], rows[g], seen);
        CHECK(s.pos.size() == s.slot.size());
        std::set<int64_t> of1;
        for (size_t i = 0; i < s.pos.size(); ++i) {
            CHECK(s.pos[i] >= 0 && s.pos[i] < rows[g]);                    // never a position the shard does not hold
            CHECK(s.slot[i] == 0 || s.slot[i] == 1);
            if (s.slot[i] == 0) { CHECK(s.pos[i] == got0 - base[g]); ++got0; }
            else of1.insert(s.pos[i] + base[g]);
        }
        std::set<int64_t> want1;
        for (int64_t k : s1)
            if (k >= base[g] && k < base[g] + rows[g]) want1.insert(k);
        CHECK(of1 == want1);
        if (rows[g] == 0) CHECK(s.pos.empty());
    }
    CHECK(got0 == total);
    // the row behind a border is position 0 of the next shard that holds rows, the row in front the last of the one before
    const Seen a = seen_of_shard(base[2], rows[2], {&s1});
    CHECK((a.pos == std::vector<int64_t>{0, 0, 2}));                       // key 5 twice (borders 1 and 2 coincide: shard 1 is empty), key 7
    const Seen b = seen_of_shard(base[3], rows[3], {&s1});
    CHECK((b.pos == std::vector<int64_t>{0, 0}));                          // key 8: behind border 3 and in front of border 4
}

// ---- the shares of a limit -----------------------------------------------------------------------------------------------------
static int64_t brute_prefix(int64_t limit, const std::vector<std::vector<uint8_t>> &dead, size_t g)
{
    // rows of shard g among the first max(1, limit) live rows of the concatenation, as a position behind the last of them
    int64_t live = 0, end = 0;
    const int64_t want = std::max<int64_t>(1, limit);
    for (size_t s = 0; s <= g; ++s)
        for (size_t p = 0; p < dead[s].size(); ++p) {
            if (dead[s][p]) continue;
            if (live >= want) return s == g ? end : 0;
            ++live;
            if (s == g) end = (int64_t)p + 1;
        }
    return end;
}

static void test_shares()
{
    // three shards of 6, 0 and 5 rows; deleted: rows 1 and 4 of shard 0, rows 0 and 3 of shard 2
    const std::vector<std::vector<uint8_t>> dead{{0, 1, 0, 0, 1, 0}, {}, {1, 0, 0, 1, 0}};
    std::vector<std::vector<int64_t>> dpos(dead.size());
    std::vector<int64_t> base(dead.size()), before(dead.size());
    int64_t at = 0, db = 0;
    for (size_t g = 0; g < dead.size(); ++g) {
        base[g] = at; before[g] = db;
        for (size_t p = 0; p < dead[g].size(); ++p)
            if (dead[g][p]) dpos[g].push_back((int64_t)p);
        at += (int64_t)dead[g].size(); db += (int64_t)dpos[g].size();
    }
    auto share = [&](int64_t limit, size_t g) { return prefix_rows(limit, base[g], before[g], (int64_t)dead[g].size(), dpos[g].data(), dpos[g].size()); };
    CHECK(share(3, 0) == 4 && share(3, 2) == 0);                           // ends inside shard 0: live rows 0, 2, 3
    CHECK(share(4, 0) == 6 && share(4, 2) == 0);                           // exactly at the border: the 4 live rows of shard 0
    CHECK(share(5, 0) == 6 && share(5, 2) == 2);                           // one row beyond it, with a deleted row in front: positions 0, 1
    CHECK(share(7, 2) == 5 && share(8, 2) == 5 && share(1000, 2) == 5);    // the last live row, and beyond the last row
    CHECK(share(0, 0) == 1 && share(-5, 0) == 1);                          // Take(Math.Max(1, maxCount))
    for (int64_t limit = -2; limit <= 14; ++limit)
        for (size_t g = 0; g < dead.size(); ++g) {
            const int64_t want = brute_prefix(limit, dead, g), got = share(limit, g);
            // (a prefix may end behind trailing deleted rows or in front of them: the live rows below it are what counts)
            int64_t lw = 0, lg = 0;
            for (int64_t p = 0; p < (int64_t)dead[g].size(); ++p) { if (!dead[g][(size_t)p] && p < want) ++lw; if (!dead[g][(size_t)p] && p < got) ++lg; }
            CHECK(lw == lg);
        }
    // with a scope: the split's took, the part empty, whole or clipped
    const std::vector<int64_t> live{4, 0, 3};
    const cscope::Split in = cscope::split_limit(live, 3);                 // ends inside shard 0
    CHECK(scope_share(in, 0, 4).part == Part::Clipped && scope_share(in, 0, 4).took == 3);
    CHECK(scope_share(in, 1, 0).part == Part::Empty && scope_share(in, 2, 3).part == Part::Empty);
    const cscope::Split edge = cscope::split_limit(live, 4);               // exactly at the border
    CHECK(scope_share(edge, 0, 4).part == Part::Whole && scope_share(edge, 2, 3).part == Part::Empty);
    const cscope::Split next = cscope::split_limit(live, 5);
    CHECK(scope_share(next, 2, 3).part == Part::Clipped && scope_share(next, 2, 3).took == 1);
    const cscope::Split all = cscope::split_limit(live, 1000);             // beyond the last row
    CHECK(scope_share(all, 0, 4).part == Part::Whole && scope_share(all, 1, 0).part == Part::Empty && scope_share(all, 2, 3).part == Part::Whole);
    CHECK(scope_share(all, 2, 3).took == 3);
}

// ---- the order of the holds ----------------------------------------------------------------------------------------------------
static void test_holds()
{
    const std::vector<uintptr_t> keys{100, 50, 70}, scope{90, 60, 10};
    const std::vector<Hold> h = holds(keys, scope);
    const std::vector<Hold> want{{0, 1}, {0, 0}, {1, 0}, {1, 1}, {2, 1}, {2, 0}};
    CHECK(h == want);
    const std::vector<Hold> alone = holds(keys, {});
    CHECK((alone == std::vector<Hold>{{0, 0}, {1, 0}, {2, 0}}));
    CHECK(holds({}, {}).empty());
    // one total order: (shard, address) ascending, whatever the call
    for (const auto &hs : {h, alone})
        for (size_t i = 1; i < hs.size(); ++i) {
            const uintptr_t a = hs[i - 1].which ? scope[(size_t)hs[i - 1].shard] : keys[(size_t)hs[i - 1].shard];
            const uintptr_t b = hs[i].which ? scope[(size_t)hs[i].shard] : keys[(size_t)hs[i].shard];
            CHECK(hs[i - 1].shard < hs[i].shard || (hs[i - 1].shard == hs[i].shard && a < b));
        }
}

// ---- random placements: the rounds over the split state keep what one walk keeps on the concatenation ---------------------------
static void test_random()
{
    std::mt19937_64 rng(20240607);
    long placements = 0, rounds_run = 0, multi = 0, cut = 0;
    for (int trial = 0; trial < 2000; ++trial) {
        const int32_t G = 1 + (int32_t)(rng() % 5);
        std::vector<int64_t> rows((size_t)G);
        for (auto &r : rows) r = (rng() % 4 == 0) ? 0 : (int64_t)(rng() % 60);
        const std::vector<int64_t> base = bases_of(rows);
        const int64_t n = base.back() + rows.back();
        const int32_t n_keys = 1 + (int32_t)(rng() % 12);
        const bool scoped = rng() % 2 == 0;
        const int64_t run = rng() % 2 == 0 ? 0 : 2 + (int64_t)(rng() % 9);
        std::vector<int64_t> key((size_t)n), rank((size_t)n);
        std::vector<uint8_t> dead((size_t)n), in_scope((size_t)n);
        std::iota(rank.begin(), rank.end(), 0);
        std::shuffle(rank.begin(), rank.end(), rng);                       // rank[row]: the smaller, the better
        for (int64_t r = 0; r < n; ++r) {
            // spread: a few keys at random; concentrated: the best rows share keys in runs, so a pool fills with closed keys
            key[(size_t)r] = rng() % 16 == 0 ? per_key::kNone : run ? rank[(size_t)r] / run : (int64_t)(rng() % (uint64_t)n_keys);
            dead[(size_t)r] = rng() % 10 == 0;
            in_scope[(size_t)r] = !scoped || rng() % 3 != 0;
        }
        const int64_t limit = (int64_t)(rng() % (uint64_t)(n + 6)) - 1;
        const int32_t pool = 1 + (int32_t)(rng() % 8), take = rng() % 2 ? pool : 1 + (int32_t)(rng() % (uint64_t)pool), m = rng() % 2 ? 1 : 1 + (int32_t)(rng() % 3);
        // ---- the concatenation: one index, one walk
        std::vector<int64_t> cand;
        for (int64_t r = 0; r < n && (int64_t)cand.size() < std::max<int64_t>(1, limit); ++r)
            if (!dead[(size_t)r] && in_scope[(size_t)r]) cand.push_back(r);
        std::vector<int64_t> ranking = cand;
        std::sort(ranking.begin(), ranking.end(), [&](int64_t a, int64_t b) { return rank[(size_t)a] < rank[(size_t)b]; });
        std::vector<int64_t> rkeys;
        for (int64_t r : ranking) rkeys.push_back(key[(size_t)r]);
        std::vector<int64_t> want;
        for (int32_t i : per_key::walk_all((int32_t)ranking.size(), rkeys.data(), take, m)) want.push_back(ranking[(size_t)i]);
        // ---- the split state: every shard's frozen part by its share
        std::vector<std::vector<uint8_t>> frozen((size_t)G);
        std::vector<int64_t> live((size_t)G, 0);
        for (int32_t g = 0; g < G; ++g)
            for (int64_t p = 0; p < rows[(size_t)g]; ++p)
                if (!dead[(size_t)(base[(size_t)g] + p)] && in_scope[(size_t)(base[(size_t)g] + p)]) live[(size_t)g] += 1;
        const cscope::Split split = cscope::split_limit(live, limit);
        int64_t dead_before = 0, frozen_rows = 0;
        for (int32_t g = 0; g < G; ++g) {
            const int64_t b = base[(size_t)g], nr = rows[(size_t)g];
            frozen[(size_t)g].assign((size_t)nr, 0);
            std::vector<int64_t> dpos;
            for (int64_t p = 0; p < nr; ++p)
                if (dead[(size_t)(b + p)]) dpos.push_back(p);
            if (!scoped) {
                const int64_t end = prefix_rows(limit, b, dead_before, nr, dpos.data(), dpos.size());
                for (int64_t p = 0; p < end; ++p) frozen[(size_t)g][(size_t)p] = !dead[(size_t)(b + p)];
                if (end > 0 && end < nr) ++cut;
            } else {
                const Share sh = scope_share(split, g, live[(size_t)g]);
                int64_t set = 0;
                for (int64_t p = 0; p < nr && sh.part != Part::Empty; ++p) {
                    if (dead[(size_t)(b + p)] || !in_scope[(size_t)(b + p)]) continue;
                    if (sh.part == Part::Clipped && set >= sh.took) break;
                    frozen[(size_t)g][(size_t)p] = 1; ++set;
                }
                if (sh.part == Part::Clipped) ++cut;
            }
            for (uint8_t f : frozen[(size_t)g]) frozen_rows += f;
            dead_before += (int64_t)dpos.size();
        }
        CHECK(frozen_rows == (int64_t)cand.size());
        // ---- the rounds
        per_key::State st;
        std::vector<int64_t> kept;
        for (int32_t round = 1; !st.finished; ++round) {
            CHECK(round <= take);
            std::vector<int64_t> tk;
            std::vector<uint64_t> tm;
            per_key::build_table({&st.closed}, tk, tm);                    // the same table on every shard
            std::vector<int64_t> found;
            for (int32_t g = 0; g < G; ++g) {
                std::vector<uint8_t> bits = frozen[(size_t)g];
                for (int64_t p = 0; p < rows[(size_t)g]; ++p)
                    if (per_key::slot_closed(per_key::table_mask(tk.data(), tm.data(), (int32_t)tk.size(), key[(size_t)(base[(size_t)g] + p)]), 0)) bits[(size_t)p] = 0;
                const Seen seen = seen_of_shard(base[(size_t)g], rows[(size_t)g], {&st.seen});
                for (size_t i = 0; i < seen.pos.size(); ++i) {
                    CHECK(seen.pos[i] >= 0 && seen.pos[i] < rows[(size_t)g] && seen.slot[i] == 0);
                    bits[(size_t)seen.pos[i]] = 0;
                }
                for (int64_t p = 0; p < rows[(size_t)g]; ++p)
                    if (bits[(size_t)p]) found.push_back(base[(size_t)g] + p);
            }
            std::sort(found.begin(), found.end(), [&](int64_t a, int64_t b) { return rank[(size_t)a] < rank[(size_t)b]; });
            if ((int32_t)found.size() > pool) found.resize((size_t)pool);
            const int32_t cnt = (int32_t)found.size();
            std::vector<int64_t> okeys((size_t)pool, -1), rk((size_t)pool, per_key::kNone);
            std::copy(found.begin(), found.end(), okeys.begin());
            const Gather gp = gather_plan(base, rows, 1, pool, okeys.data(), &cnt);
            CHECK(gp.ok);
            size_t gathered = 0;
            for (int32_t g = 0; g < G; ++g)
                for (size_t i = 0; i < gp.pos[(size_t)g].size(); ++i, ++gathered)
                    rk[(size_t)gp.at[(size_t)g][i]] = key[(size_t)(base[(size_t)g] + gp.pos[(size_t)g][i])];   // the shard's own column
            CHECK(gathered == (size_t)cnt);
            std::vector<int32_t> number((size_t)pool);
            std::iota(number.begin(), number.end(), 0);
            const size_t had = st.kept.size();
            per_key::walk_round(st, cnt, rk.data(), okeys.data(), number.data(), take, m, pool);
            for (size_t t = had; t < st.kept.size(); ++t) kept.push_back(okeys[(size_t)st.kept[t]]);
            if (!st.finished) CHECK(st.kept.size() > had);
            ++rounds_run;
        }
        CHECK(kept == want);
        if (st.rounds > 1) ++multi;
        ++placements;
    }
    printf("random placements: %ld, %ld rounds, %ld with more than one round, %ld shares that end inside a shard\n", placements, rounds_run, multi, cut);
    CHECK(placements == 2000 && multi > 300 && cut > 500);
}

int main()
{
    test_gather();
    test_seen();
    test_shares();
    test_holds();
    test_random();
    printf("checks: %ld\n", g_checks);
    printf("orr_cluster_per_key_plan_selftest: ok\n");
    return 0;
}
