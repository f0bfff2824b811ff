// orr_cluster_group_plan_selftest -- the host rules of orr_cluster_group_plan.h on the CPU (no HIP, no GPU): the groups of a call
// as its distinct handles; the lock order over several handles, against the property that makes it safe (one total order over
// all locks, each taken once, and the order of an edit a sub-order of it); the split per group against a row-by-row walk of the
// global candidate order; which groups are used and which k' total the first rung takes; and where every query goes after
// the first rung.
// Exit status 0 and a last line "orr_cluster_group_plan_selftest: ok" when everything holds;
// tests/test_cluster_group_cpu.py runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../orr_cluster_group_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

// ---- distinct: every listed scope maps to the group of its handle; the groups are the handles in order of first appearance --
static void test_distinct()
{
    {
        const cgroup::Distinct d = cgroup::distinct({0x100, 0x200, 0x100, 0x300, 0x200});
        CHECK(d.first == (std::vector<int32_t>{0, 1, 3}));
        CHECK(d.group_of == (std::vector<int32_t>{0, 1, 0, 2, 1}));
        CHECK(cgroup::distinct({0x100}).first.size() == 1);
        CHECK(cgroup::distinct({}).first.empty());
    }
    std::mt19937_64 rng(5);
    for (int it = 0; it < 500; ++it) {
        const size_t n = 1 + rng() % 64;
        std::vector<uintptr_t> h(n);
        for (auto &x : h) x = 0x1000 + 0x40 * (rng() % 12);
        const cgroup::Distinct d = cgroup::distinct(h);
        std::set<uintptr_t> seen;
        std::vector<uintptr_t> order;                          // brute force: first appearances
        for (uintptr_t x : h)
            if (seen.insert(x).second) order.push_back(x);
        CHECK(d.first.size() == order.size());
        for (size_t g = 0; g < d.first.size(); ++g) CHECK(h[(size_t)d.first[g]] == order[g]);
        for (size_t i = 0; i < n; ++i) {
            CHECK(d.group_of[i] >= 0 && (size_t)d.group_of[i] < order.size());
            CHECK(order[(size_t)d.group_of[i]] == h[i]);       // the same handle, hence held once
        }
    }
}

// ---- holds: one strict total order over (shard, address); every part once; an edit's order is a sub-order -----------------
static void test_holds()
{
    std::mt19937_64 rng(7);
    for (int it = 0; it < 400; ++it) {
        const size_t D = 1 + rng() % 10, S = 1 + rng() % 6;
        std::vector<std::vector<uintptr_t>> parts(D, std::vector<uintptr_t>(S));
        std::vector<uintptr_t> pool;
        for (size_t i = 0; i < D * S; ++i) pool.push_back(0x10000 + 0x80 * i);
        std::shuffle(pool.begin(), pool.end(), rng);
        for (size_t d = 0; d < D; ++d)
            for (size_t s = 0; s < S; ++s) parts[d][s] = pool[d * S + s];
        const std::vector<cgroup::Hold> h = cgroup::holds(parts);
        CHECK(h.size() == D * S);
        std::set<std::pair<int32_t, int32_t>> once;
        for (size_t i = 0; i < h.size(); ++i) {
            CHECK(once.insert({h[i].shard, h[i].group}).second);
            if (i == 0) continue;
            const std::pair<int32_t, uintptr_t> a{h[i - 1].shard, parts[(size_t)h[i - 1].group][(size_t)h[i - 1].shard]};
            const std::pair<int32_t, uintptr_t> b{h[i].shard, parts[(size_t)h[i].group][(size_t)h[i].shard]};
            CHECK(a < b);                                      // strictly ascending in (shard, address): one total order
        }
        // an edit of two of the handles (chandle::holds: combine) takes its locks in an order this one contains
        if (D >= 2) {
            const size_t x = rng() % D, y = (x + 1 + rng() % (D - 1)) % D;
            const std::vector<chandle::Hold> e = chandle::holds(parts[x], parts[y], true);
            size_t at = 0;
            for (const chandle::Hold &eh : e) {
                const uintptr_t want = eh.which == 0 ? parts[x][(size_t)eh.shard] : parts[y][(size_t)eh.shard];
                while (at < h.size() && parts[(size_t)h[at].group][(size_t)h[at].shard] != want) ++at;
                CHECK(at < h.size());                          // found behind the previous one
            }
        }
        // two searches over overlapping sets of handles, listed in different orders, take the shared parts in the same order
        std::vector<size_t> perm(D);
        for (size_t d = 0; d < D; ++d) perm[d] = d;
        std::shuffle(perm.begin(), perm.end(), rng);
        std::vector<std::vector<uintptr_t>> other;
        for (size_t d = 0; d < D; ++d) other.push_back(parts[perm[d]]);
        const std::vector<cgroup::Hold> h2 = cgroup::holds(other);
        CHECK(h2.size() == h.size());
        for (size_t i = 0; i < h.size() && i < h2.size(); ++i)
            CHECK(parts[(size_t)h[i].group][(size_t)h[i].shard] == other[(size_t)h2[i].group][(size_t)h2[i].shard]);
    }
    // the same part under two groups: held once
    const std::vector<cgroup::Hold> h = cgroup::holds({{0x100, 0x300}, {0x100, 0x200}});
    CHECK(h.size() == 3);
    CHECK((h[0] == cgroup::Hold{0, 0}) && (h[1] == cgroup::Hold{1, 1}) && (h[2] == cgroup::Hold{1, 0}));
    CHECK(cgroup::holds({}).empty());
}

// ---- splits: per group, against a walk of the group's rows in the global candidate order -----------------------------------
static void test_splits()
{
    std::mt19937_64 rng(9);
    for (int it = 0; it < 300; ++it) {
        const size_t D = 1 + rng() % 8, S = 1 + rng() % 5;
        std::vector<std::vector<int64_t>> live(D, std::vector<int64_t>(S));
        for (auto &l : live)
            for (auto &x : l) x = rng() % 4 == 0 ? 0 : (int64_t)(rng() % 50);
        const int64_t limit = (int64_t)(rng() % 120) - 5;      // (<= 0: one row, as Take(Math.Max(1, maxCount)))
        std::vector<cscope::Split> sp;
        CHECK(cgroup::splits(live, limit, sp));
        CHECK(sp.size() == D);
        for (size_t d = 0; d < D; ++d) {
            std::vector<int64_t> took(S, 0), before(S, 0);
            int64_t walked = 0;
            for (size_t s = 0; s < S; ++s) {
                before[s] = walked;
                for (int64_t r = 0; r < live[d][s]; ++r, ++walked)
                    if (walked < std::max<int64_t>(1, limit)) took[s] += 1;
            }
            CHECK(sp[d].took == took && sp[d].before == before);
            for (size_t s = 0; s < S; ++s) CHECK(cscope::shard_took(live[d][s], limit, before[s]) == took[s]);    // what the shard form works out
        }
    }
    std::vector<cscope::Split> sp;
    CHECK(!cgroup::splits({{3, 4}, {5, -1}}, 10, sp));        // an orphaned part: nothing is split
}

// ---- first + route -----------------------------------------------------------------------------------------------------------
static void test_first_and_route()
{
    std::mt19937_64 rng(13);
    for (int it = 0; it < 300; ++it) {
        const size_t D = 1 + rng() % 8, S = 1 + rng() % 4, B = 1 + rng() % 40;
        std::vector<std::vector<int64_t>> live(D, std::vector<int64_t>(S));
        for (auto &l : live) {
            const bool empty = rng() % 3 == 0;
            for (auto &x : l) x = empty ? 0 : (int64_t)(rng() % 50);
        }
        std::vector<cscope::Split> sp;
        CHECK(cgroup::splits(live, 1 + (int64_t)(rng() % 100), sp));
        std::vector<int32_t> qg(B);
        for (auto &g : qg) g = (int32_t)(rng() % D);
        const cgroup::First f = cgroup::first(sp, qg);
        std::set<int32_t> used;
        int64_t total = 0;
        std::vector<int32_t> ids;
        for (size_t b = 0; b < B; ++b)
            if (sp[(size_t)qg[b]].total > 0) { used.insert(qg[b]); ids.push_back((int32_t)b); total = std::max(total, sp[(size_t)qg[b]].total); }
        CHECK(f.n_used == (int32_t)used.size() && f.ids == ids && f.total == total);
        CHECK((f.only >= 0) == (used.size() == 1));
        if (used.size() == 1) CHECK(f.only == *used.begin());
        for (size_t g = 0; g < D; ++g) CHECK((f.used[g] != 0) == (used.count((int32_t)g) != 0));
        // route: certified queries are final, the others gather under their own group, ascending, each once
        std::vector<uint8_t> cert(ids.size());
        for (auto &c : cert) c = rng() % 3 != 0;
        std::vector<std::vector<int32_t>> again(D);
        cgroup::route(ids, cert, qg, again);
        size_t n_again = 0;
        for (size_t g = 0; g < D; ++g) {
            CHECK(std::is_sorted(again[g].begin(), again[g].end()));
            for (int32_t b : again[g]) {
                CHECK(qg[(size_t)b] == (int32_t)g);
                const size_t i = (size_t)(std::find(ids.begin(), ids.end(), b) - ids.begin());
                CHECK(i < ids.size() && !cert[i]);
            }
            n_again += again[g].size();
        }
        CHECK(n_again == (size_t)std::count(cert.begin(), cert.end(), (uint8_t)0));
    }
}

int main()
{
    test_distinct();
    test_holds();
    test_splits();
    test_first_and_route();
    if (g_failed) { printf("orr_cluster_group_plan_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("orr_cluster_group_plan_selftest: ok\n");
    return 0;
}
