// orr_cluster_diverse_plan_selftest -- the host plan of the cluster diverse search's pair step (orr_cluster_diverse_plan.h)
// against brute-force restatements, on a machine without a GPU.  tests/test_cluster_diverse_cpu.py runs it.
#include "../orr_cluster_diverse_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

using namespace cdiverse;

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

// ---- locate ------------------------------------------------------------------------------------------------------------------
static void test_locate()
{
    const std::vector<int64_t> rows{5, 0, 3, 0, 0, 7, 0};                  // empty shards in the middle and at the end
    const std::vector<int64_t> base = bases_of(rows);
    int64_t key = 0;
    for (size_t g = 0; g < rows.size(); ++g)
        for (int64_t r = 0; r < rows[g]; ++r, ++key) {
            Place pl{-1, -1};
            CHECK(locate(base, rows, key, &pl) && pl.shard == (int32_t)g && pl.pos == r);
        }
    CHECK(key == 15);
    Place pl{-7, -7};
    CHECK(!locate(base, rows, 15, &pl) && !locate(base, rows, -1, &pl) && !locate(base, rows, INT64_MAX, &pl) && !locate(base, rows, INT64_MIN, &pl));
    CHECK(pl.shard == -7 && pl.pos == -7);                                 // a miss writes nothing
    CHECK(!locate({}, {}, 0, &pl));
    CHECK(!locate({0, 0}, {0, 0}, 0, &pl));                                // a cluster of empty shards
    // bases that do not start at 0 and leave a gap: a key in the gap is in no shard
    CHECK(locate({10, 20}, {4, 4}, 13, &pl) && pl.shard == 0 && pl.pos == 3);
    CHECK(!locate({10, 20}, {4, 4}, 14, &pl) && !locate({10, 20}, {4, 4}, 9, &pl));
    CHECK(locate({10, 20}, {4, 4}, 20, &pl) && pl.shard == 1 && pl.pos == 0);
    // a plan over a key outside every shard is refused and says which
    const int64_t keys[4] = {0, 14, 99, 3};
    const int32_t cnt[1] = {4};
    const uint8_t needs[1] = {1};
    const Plan p = make_plan(base, rows, 1, 4, keys, cnt, needs, 8);
    CHECK(!p.ok && p.bad_query == 0 && p.bad_key == 99 && p.lists.empty() && p.groups.empty());
}

// ---- home --------------------------------------------------------------------------------------------------------------------
static void test_home()
{
    auto home = [](std::vector<int32_t> shards, int32_t G) {
        std::vector<Place> m;
        for (int32_t s : shards) m.push_back(Place{s, 0});
        return home_of(m.data(), (int32_t)m.size(), G);
    };
    CHECK(home({2}, 3) == 2);
    CHECK(home({2, 1}, 3) == 1);                                           // a tie: the lowest shard index
    CHECK(home({2, 1, 2}, 3) == 2);
    CHECK(home({2, 2, 1, 1, 0}, 3) == 1);
    CHECK(home({0, 1, 2, 0, 1, 2}, 3) == 0);
    CHECK(home({3, 3, 0, 0, 3, 0}, 4) == 0);
    CHECK(home({7, 7, 7, 7}, 8) == 7);
    std::mt19937 rng(1);
    for (int it = 0; it < 2000; ++it) {
        const int32_t G = 1 + (int32_t)(rng() % 8), n = 1 + (int32_t)(rng() % 56);
        std::vector<int32_t> sh((size_t)n), held((size_t)G, 0);
        for (int32_t &s : sh) { s = (int32_t)(rng() % (uint32_t)G); held[(size_t)s] += 1; }
        const int32_t h = home(sh, G);
        for (int32_t g = 0; g < G; ++g) CHECK(held[(size_t)g] < held[(size_t)h] || (held[(size_t)g] == held[(size_t)h] && g >= h));
    }
}

// A plan against a restatement: every list's slots lead to the row they name, the runs carry the gather buffers into the
// staging buffers, the counts agree.  Returns the rows moved.
static int64_t verify(const Plan &p, const std::vector<int64_t> &base, const std::vector<int64_t> &rows, int32_t B, int32_t key_stride,
                      const int64_t *keys, const int32_t *cnt, const uint8_t *needs, int32_t dim, int64_t budget, int32_t per_launch)
{
    const int32_t G = (int32_t)base.size();
    CHECK(p.ok && (int32_t)p.list_of.size() == B);
    int32_t n_lists = 0, stride = 1;
    for (int32_t b = 0; b < B; ++b) {
        const bool listed = needs[b] && cnt[b] >= 1;
        CHECK((p.list_of[(size_t)b] >= 0) == listed);
        if (!listed) continue;
        CHECK(p.list_of[(size_t)b] == n_lists && p.lists[(size_t)n_lists].query == b && p.lists[(size_t)n_lists].n == cnt[b]);
        stride = std::max(stride, cnt[b]);
        ++n_lists;
    }
    CHECK((int32_t)p.lists.size() == n_lists && p.stride == stride);
    int32_t next_list = 0;
    int64_t moved_all = 0;
    for (const Group &g : p.groups) {
        CHECK(g.first == next_list && g.count >= 1);                       // consecutive, never empty
        next_list += g.count;
        CHECK((int32_t)g.gather.size() == G && (int32_t)g.staged.size() == G && (int32_t)g.lists.size() == G);
        // the transport, played on row NAMES (global order keys): gather, then the runs
        std::vector<std::vector<int64_t>> gathered((size_t)G), staging((size_t)G);
        int64_t staged_all = 0, gathered_all = 0;
        for (int32_t s = 0; s < G; ++s) {
            for (uint32_t pos : g.gather[(size_t)s]) { CHECK((int64_t)pos < rows[(size_t)s]); gathered[(size_t)s].push_back(base[(size_t)s] + pos); }
            staging[(size_t)s].assign((size_t)g.staged[(size_t)s], -1);
            staged_all += g.staged[(size_t)s];
            gathered_all += (int64_t)g.gather[(size_t)s].size();
        }
        CHECK(staged_all == g.moved && gathered_all == g.moved);
        int64_t run_rows = 0;
        for (size_t r = 0; r < g.runs.size(); ++r) {
            const Run &run = g.runs[r];
            CHECK(run.src != run.home && run.rows > 0);
            if (r > 0) CHECK(g.runs[r - 1].src < run.src || (g.runs[r - 1].src == run.src && g.runs[r - 1].home < run.home));      // one run a pair of shards
            CHECK(run.src_at >= 0 && run.src_at + run.rows <= (int64_t)gathered[(size_t)run.src].size());
            CHECK(run.home_at >= 0 && run.home_at + run.rows <= g.staged[(size_t)run.home]);
            for (int64_t k = 0; k < run.rows; ++k) {
                CHECK(staging[(size_t)run.home][(size_t)(run.home_at + k)] == -1);                   // no slot written twice
                staging[(size_t)run.home][(size_t)(run.home_at + k)] = gathered[(size_t)run.src][(size_t)(run.src_at + k)];
            }
            run_rows += run.rows;
        }
        CHECK(run_rows == g.moved);
        if (g.count > 1) CHECK(g.moved * 4 * (int64_t)dim <= budget);      // only a single list may exceed the budget
        int32_t in_homes = 0;
        for (int32_t h = 0; h < G; ++h) {
            CHECK((int32_t)g.lists[(size_t)h].size() <= per_launch);
            in_homes += (int32_t)g.lists[(size_t)h].size();
            std::vector<uint8_t> used((size_t)g.staged[(size_t)h], 0);
            int32_t before = -1;
            for (int32_t l : g.lists[(size_t)h]) {
                CHECK(l > before && l >= g.first && l < g.first + g.count);
                before = l;
                const List &li = p.lists[(size_t)l];
                CHECK(li.home == h);
                std::vector<int32_t> held((size_t)G, 0);
                int32_t foreign = 0;
                for (int32_t i = 0; i < li.n; ++i) {
                    const int64_t key = keys[(size_t)li.query * (size_t)key_stride + (size_t)i];
                    Place pl{-1, -1};
                    CHECK(locate(base, rows, key, &pl));
                    held[(size_t)pl.shard] += 1;
                    const bool f = (li.foreign >> i) & 1;
                    CHECK(f == (pl.shard != h));
                    if (f) {
                        CHECK((int64_t)li.at[(size_t)i] < g.staged[(size_t)h] && staging[(size_t)h][li.at[(size_t)i]] == key);
                        CHECK(!used[li.at[(size_t)i]]);                    // a row wanted twice is staged twice
                        used[li.at[(size_t)i]] = 1;
                        ++foreign;
                    } else {
                        CHECK(base[(size_t)h] + (int64_t)li.at[(size_t)i] == key);
                    }
                }
                CHECK((li.foreign >> li.n) == 0);
                for (int32_t s = 0; s < G; ++s) CHECK(held[(size_t)s] < held[(size_t)h] || (held[(size_t)s] == held[(size_t)h] && s >= h));
                CHECK(foreign == li.n - held[(size_t)h] && foreign <= foreign_bound(li.n, G));
            }
            for (uint8_t u : used) CHECK(u == 1);                          // nothing staged that no list reads
        }
        CHECK(in_homes == g.count);
        moved_all += g.moved;
    }
    CHECK(next_list == n_lists && moved_all == p.moved);
    // a group ends only for a reason: the next list would break the budget or its home's launch
    for (size_t gi = 0; gi + 1 < p.groups.size(); ++gi) {
        const Group &g = p.groups[gi];
        const List &nx = p.lists[(size_t)(g.first + g.count)];
        int64_t f = 0;
        for (int32_t i = 0; i < nx.n; ++i) f += (nx.foreign >> i) & 1;
        CHECK((g.moved + f) * 4 * (int64_t)dim > budget || (int32_t)g.lists[(size_t)nx.home].size() == per_launch);
    }
    return moved_all;
}

// ---- the bound n - ceil(n / G), met exactly by an even spread --------------------------------------------------------------
static void test_bound()
{
    for (int32_t G = 1; G <= 8; ++G) {
        const std::vector<int64_t> rows((size_t)G, 100);
        const std::vector<int64_t> base = bases_of(rows);
        for (int32_t n = 0; n <= 56; ++n) {
            CHECK(foreign_bound(n, G) == n - (n + G - 1) / G);
            std::vector<int64_t> keys((size_t)std::max(n, 1));
            for (int32_t i = 0; i < n; ++i) keys[(size_t)i] = base[(size_t)(i % G)] + i / G;       // spread evenly: the worst case
            const int32_t cnt[1] = {n};
            const uint8_t needs[1] = {1};
            const Plan p = make_plan(base, rows, 1, std::max(n, 1), keys.data(), cnt, needs, 16);
            const int64_t moved = verify(p, base, rows, 1, std::max(n, 1), keys.data(), cnt, needs, 16, kStageBudgetBytes, kListsPerLaunch);
            CHECK(moved == foreign_bound(n, G));
            if (n > 0) CHECK(p.lists[0].home == 0);                        // the even spread's tie
            // on one shard: no list of positions to gather, no run, nothing staged
            for (int32_t i = 0; i < n; ++i) keys[(size_t)i] = base[(size_t)(G - 1)] + (n - 1 - i);
            const Plan q = make_plan(base, rows, 1, std::max(n, 1), keys.data(), cnt, needs, 16);
            CHECK(verify(q, base, rows, 1, std::max(n, 1), keys.data(), cnt, needs, 16, kStageBudgetBytes, kListsPerLaunch) == 0);
            for (const Group &g : q.groups) {
                CHECK(g.runs.empty());
                for (int32_t s = 0; s < G; ++s) CHECK(g.gather[(size_t)s].empty() && g.staged[(size_t)s] == 0);
            }
            CHECK((n == 0) == q.groups.empty());
        }
    }
}

// ---- the slot numbering, by hand -------------------------------------------------------------------------------------------
static void test_slots()
{
    const std::vector<int64_t> rows{10, 0, 10, 10};
    const std::vector<int64_t> base = bases_of(rows);                      // 0, 10, 10, 20
    // query 0: home 2 (3 of 5), foreign from shard 0 (key 4) and shard 3 (key 25); query 1 reads no cosine;
    // query 2: home 0 (tie 2 : 2 with shard 3), foreign keys 21, 21 (the same row twice); query 3: home 2, foreign key 4 again
    const int64_t keys[4 * 5] = {12, 4, 13, 25, 19, /**/ 0, 1, 2, 3, 4, /**/ 21, 3, 21, 7, -1, /**/ 4, 11, 15, -1, -1};
    const int32_t cnt[4] = {5, 5, 4, 3};
    const uint8_t needs[4] = {1, 0, 1, 1};
    const Plan p = make_plan(base, rows, 4, 5, keys, cnt, needs, 4);
    CHECK(verify(p, base, rows, 4, 5, keys, cnt, needs, 4, kStageBudgetBytes, kListsPerLaunch) == 5);
    CHECK(p.lists.size() == 3 && p.groups.size() == 1 && p.stride == 5);
    CHECK(p.list_of == (std::vector<int32_t>{0, -1, 1, 2}));
    const Group &g = p.groups[0];
    CHECK(p.lists[0].home == 2 && p.lists[0].foreign == 0b01010 && p.lists[1].home == 0 && p.lists[1].foreign == 0b0101 && p.lists[2].home == 2 && p.lists[2].foreign == 0b001);
    // source 0 gathers for home 2: key 4 (list 0), key 4 (list 2); source 3 gathers for home 0: 21, 21, then for home 2: 25
    CHECK(g.gather[0] == (std::vector<uint32_t>{4, 4}) && g.gather[1].empty() && g.gather[2].empty() && g.gather[3] == (std::vector<uint32_t>{1, 1, 5}));
    CHECK(g.staged == (std::vector<int64_t>{2, 0, 3, 0}));
    // home 2's staging: source 0's rows first (slots 0, 1), then source 3's (slot 2)
    CHECK(p.lists[0].at[0] == 2 && p.lists[0].at[1] == 0 && p.lists[0].at[2] == 3 && p.lists[0].at[3] == 2 && p.lists[0].at[4] == 9);
    CHECK(p.lists[1].at[0] == 0 && p.lists[1].at[1] == 3 && p.lists[1].at[2] == 1 && p.lists[1].at[3] == 7);
    CHECK(p.lists[2].at[0] == 1 && p.lists[2].at[1] == 1 && p.lists[2].at[2] == 5);
    CHECK(g.runs.size() == 3);
    CHECK(g.runs[0].src == 0 && g.runs[0].home == 2 && g.runs[0].src_at == 0 && g.runs[0].home_at == 0 && g.runs[0].rows == 2);
    CHECK(g.runs[1].src == 3 && g.runs[1].home == 0 && g.runs[1].src_at == 0 && g.runs[1].home_at == 0 && g.runs[1].rows == 2);
    CHECK(g.runs[2].src == 3 && g.runs[2].home == 2 && g.runs[2].src_at == 2 && g.runs[2].home_at == 2 && g.runs[2].rows == 1);
    CHECK(g.lists[0] == (std::vector<int32_t>{1}) && g.lists[2] == (std::vector<int32_t>{0, 2}) && g.lists[1].empty() && g.lists[3].empty());
    // no query reads a cosine: no list, no group
    const uint8_t none[4] = {0, 0, 0, 0};
    const Plan q = make_plan(base, rows, 4, 5, keys, cnt, none, 4);
    CHECK(q.ok && q.lists.empty() && q.groups.empty() && q.moved == 0 && q.list_of == (std::vector<int32_t>{-1, -1, -1, -1}));
    // ... and its keys are not even looked at
    const int64_t wild[2] = {1000, -5};
    const int32_t c2[1] = {2};
    CHECK(make_plan(base, rows, 1, 2, wild, c2, none, 4).ok);
}

// ---- groups ------------------------------------------------------------------------------------------------------------------
static void test_groups()
{
    const std::vector<int64_t> rows{1000, 1000, 1000};
    const std::vector<int64_t> base = bases_of(rows);
    const int32_t B = 40, n = 9, dim = 8;                                   // a staged row is 32 bytes
    std::vector<int64_t> keys((size_t)B * n);
    std::vector<int32_t> cnt((size_t)B, n);
    std::vector<uint8_t> needs((size_t)B, 1);
    for (int32_t b = 0; b < B; ++b)
        for (int32_t i = 0; i < n; ++i) keys[(size_t)b * n + i] = base[(size_t)(i % 3)] + b * 9 + i;     // 3 : 3 : 3 -> 6 foreign rows a query
    // 6 rows x 32 bytes = 192 bytes a query: a budget of 1000 bytes holds 5 queries
    Plan p = make_plan(base, rows, B, n, keys.data(), cnt.data(), needs.data(), dim, 1000, kListsPerLaunch);
    CHECK(verify(p, base, rows, B, n, keys.data(), cnt.data(), needs.data(), dim, 1000, kListsPerLaunch) == 6 * B);
    CHECK(p.groups.size() == 8);
    for (const Group &g : p.groups) CHECK(g.count == 5 && g.moved == 30);
    // a budget below one query's rows: every query a group of its own, each over the budget alone
    p = make_plan(base, rows, B, n, keys.data(), cnt.data(), needs.data(), dim, 100, kListsPerLaunch);
    CHECK(verify(p, base, rows, B, n, keys.data(), cnt.data(), needs.data(), dim, 100, kListsPerLaunch) == 6 * B);
    CHECK((int32_t)p.groups.size() == B);
    for (const Group &g : p.groups) CHECK(g.count == 1 && g.moved * 32 > 100);
    p = make_plan(base, rows, B, n, keys.data(), cnt.data(), needs.data(), dim, 0, kListsPerLaunch);
    CHECK((int32_t)p.groups.size() == B);
    // the launch limit per home: 7 lists a home
    p = make_plan(base, rows, B, n, keys.data(), cnt.data(), needs.data(), dim, kStageBudgetBytes, 7);
    verify(p, base, rows, B, n, keys.data(), cnt.data(), needs.data(), dim, kStageBudgetBytes, 7);
    CHECK(p.groups.size() == 6 && p.groups[0].count == 7 && p.groups[5].count == 5);               // every list's home is shard 0
    // the default limits: 2500 lists, all at home on shard 1 with nothing foreign -- 1024, 1024, 452
    const int32_t B2 = 2500;
    std::vector<int64_t> k2((size_t)B2 * 2);
    std::vector<int32_t> c2((size_t)B2, 2);
    std::vector<uint8_t> n2((size_t)B2, 1);
    for (int32_t b = 0; b < B2; ++b) { k2[(size_t)b * 2] = 1000 + b % 1000; k2[(size_t)b * 2 + 1] = 1000 + (b + 1) % 1000; }
    p = make_plan(base, rows, B2, 2, k2.data(), c2.data(), n2.data(), 1024);
    CHECK(verify(p, base, rows, B2, 2, k2.data(), c2.data(), n2.data(), 1024, kStageBudgetBytes, kListsPerLaunch) == 0);
    CHECK(p.groups.size() == 3 && p.groups[0].count == 1024 && p.groups[1].count == 1024 && p.groups[2].count == 452);
    // homes alternate: the limit holds per home, so a group holds up to 2048 lists of two homes
    for (int32_t b = 0; b < B2; ++b) { const int64_t at = (b % 2) * 2000; k2[(size_t)b * 2] = at + b % 1000; k2[(size_t)b * 2 + 1] = at + (b + 1) % 1000; }
    p = make_plan(base, rows, B2, 2, k2.data(), c2.data(), n2.data(), 1024);
    verify(p, base, rows, B2, 2, k2.data(), c2.data(), n2.data(), 1024, kStageBudgetBytes, kListsPerLaunch);
    CHECK(p.groups.size() == 2 && p.groups[0].count == 2048 && p.groups[1].count == 452);
    CHECK(kStageBudgetBytes == (64ll << 20) && kListsPerLaunch == 1024);
}

// ---- random placements -------------------------------------------------------------------------------------------------------
static void test_random()
{
    std::mt19937_64 rng(20);
    long lists = 0, groups = 0, moved = 0;
    for (int it = 0; it < 400; ++it) {
        const int32_t G = 1 + (int32_t)(rng() % 8);
        std::vector<int64_t> rows((size_t)G);
        int64_t total = 0;
        for (int64_t &r : rows) { r = rng() % 4 == 0 ? 0 : 1 + (int64_t)(rng() % 300); total += r; }
        if (total == 0) { rows[(size_t)(G - 1)] = 17; total = 17; }
        const std::vector<int64_t> base = bases_of(rows);
        const int32_t B = 1 + (int32_t)(rng() % 48), stride = 56, dim = 1 + (int32_t)(rng() % 64);
        std::vector<int64_t> keys((size_t)B * stride, -1);
        std::vector<int32_t> cnt((size_t)B);
        std::vector<uint8_t> needs((size_t)B);
        for (int32_t b = 0; b < B; ++b) {
            cnt[(size_t)b] = (int32_t)(rng() % 57);
            needs[(size_t)b] = rng() % 5 != 0;
            const int64_t centre = (int64_t)(rng() % (uint64_t)total);      // pools cluster in the global order, as hybrid scores make them
            for (int32_t i = 0; i < cnt[(size_t)b]; ++i) {
                int64_t k = rng() % 3 == 0 ? (int64_t)(rng() % (uint64_t)total) : centre + (int64_t)(rng() % 64) - 32;
                keys[(size_t)b * stride + i] = std::min<int64_t>(std::max<int64_t>(k, 0), total - 1);
            }
        }
        const int64_t budget = rng() % 2 ? kStageBudgetBytes : (int64_t)(rng() % 20000);
        const int32_t per = rng() % 2 ? kListsPerLaunch : 1 + (int32_t)(rng() % 9);
        const Plan p = make_plan(base, rows, B, stride, keys.data(), cnt.data(), needs.data(), dim, budget, per);
        moved += verify(p, base, rows, B, stride, keys.data(), cnt.data(), needs.data(), dim, budget, per);
        lists += (long)p.lists.size();
        groups += (long)p.groups.size();
    }
    printf("random placements: 400 plans, %ld lists, %ld groups, %ld rows moved\n", lists, groups, moved);
    CHECK(lists > 4000 && groups > 400 && moved > 10000);
}

int main()
{
    test_locate();
    test_home();
    test_bound();
    test_slots();
    test_groups();
    test_random();
    printf("checks: %ld\n", g_checks);
    printf("orr_cluster_diverse_plan_selftest: ok\n");
    return 0;
}
