// orr_cluster_handle_plan_selftest -- the host rules of orr_cluster_handle_plan.h on the CPU (no HIP, no GPU): where every shard
// writes its part of row_ids and when the call fails, against a buffer written row by row; the validity of a pair of cluster
// scopes; the lock order, against the property that makes it safe (one total order over all locks, each taken once); and the
// split of the limit from handle-reported counts against the split of counted lists, row by row.
// Exit status 0 and a last line "orr_cluster_handle_plan_selftest: ok" when everything holds;
// tests/test_cluster_scope_handle_cpu.py runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../orr_cluster_handle_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

// ---- row_ids: every shard writes its live rows' ids behind those of the shards in front; nothing beyond cap ----------------
// Brute force: the rows of all shards walked in the global order into a buffer with a guard behind cap.
static void check_row_ids(const std::vector<int64_t> &live, int64_t cap)
{
    const chandle::RowIdPlan p = chandle::row_id_plan(live, cap);
    std::vector<int64_t> want;                                 // (shard, r) encoded, in the global order
    for (size_t g = 0; g < live.size(); ++g)
        for (int64_t r = 0; r < live[g]; ++r) want.push_back((int64_t)g * 1000000 + r);
    CHECK(p.total == (int64_t)want.size());
    CHECK(p.fits == ((int64_t)want.size() <= cap));
    const int64_t guard = 4;
    std::vector<int64_t> buf((size_t)(cap + guard), -7);
    if (p.fits)
        for (size_t g = 0; g < live.size(); ++g)                // what the shards do, in any order
            for (int64_t r = 0; r < live[live.size() - 1 - g]; ++r) {
                const size_t sh = live.size() - 1 - g;
                buf[(size_t)(p.offset[sh] + r)] = (int64_t)sh * 1000000 + r;
            }
    for (int64_t i = 0; i < cap + guard; ++i) {
        if (p.fits && i < (int64_t)want.size()) CHECK(buf[(size_t)i] == want[(size_t)i]);
        else CHECK(buf[(size_t)i] == -7);                      // too small a cap: nothing written; never beyond cap
    }
    for (size_t g = 1; g < live.size(); ++g) CHECK(p.offset[g] == p.offset[g - 1] + live[g - 1]);
    if (!live.empty()) CHECK(p.offset[0] == 0);
}

static void test_row_ids()
{
    {
        const chandle::RowIdPlan p = chandle::row_id_plan({100, 0, 250, 80}, 430);
        CHECK(p.offset == (std::vector<int64_t>{0, 100, 100, 350}));
        CHECK(p.total == 430 && p.fits);
        CHECK(!chandle::row_id_plan({100, 0, 250, 80}, 429).fits);          // one too small
        CHECK(chandle::row_id_plan({100, 0, 250, 80}, 429).total == 430);   // ... and the count is still reported
        CHECK(chandle::row_id_plan({}, 0).fits && chandle::row_id_plan({0, 0}, 0).fits);
        CHECK(!chandle::row_id_plan({1}, -1).fits);
    }
    std::mt19937_64 rng(11);
    for (int it = 0; it < 2000; ++it) {
        std::vector<int64_t> live((size_t)(rng() % 6));
        int64_t sum = 0;
        for (int64_t &l : live) { l = rng() % 3 == 0 ? 0 : (int64_t)(rng() % 40); sum += l; }
        for (int64_t cap : {sum, sum - 1, sum + 3, (int64_t)0, (int64_t)(rng() % 100)})
            if (cap >= 0) check_row_ids(live, cap);
    }
}

// ---- combine: the pair -------------------------------------------------------------------------------------------------------
static void test_pair()
{
    int a = 0, b = 0;
    using chandle::Pair;
    CHECK(chandle::pair_valid(&a, &a, 3, 3) == Pair::Ok);
    CHECK(chandle::pair_valid(&a, &b, 3, 3) == Pair::OtherCluster);
    CHECK(chandle::pair_valid(nullptr, &a, 3, 3) == Pair::Orphaned);
    CHECK(chandle::pair_valid(&a, nullptr, 3, 3) == Pair::Orphaned);
    CHECK(chandle::pair_valid(nullptr, nullptr, 3, 3) == Pair::Orphaned);      // not "the same cluster"
    CHECK(chandle::pair_valid(&a, &a, 3, 2) == Pair::Shards);
    CHECK(chandle::pair_valid(&a, &a, 0, 0) == Pair::Shards);
    // brute force over a small world: valid exactly when both are alive, of one cluster, with equal non-zero parts
    const void *cl[3] = {nullptr, &a, &b};
    for (const void *x : cl)
        for (const void *y : cl)
            for (size_t px = 0; px < 3; ++px)
                for (size_t py = 0; py < 3; ++py)
                    CHECK((chandle::pair_valid(x, y, px, py) == Pair::Ok) == (x && y && x == y && px == py && px > 0));
}

// ---- the lock order ----------------------------------------------------------------------------------------------------------
// The key of a hold in the ONE order every call follows: (shard, address).
static std::pair<int32_t, uintptr_t> key_of(const chandle::Hold &h, const std::vector<uintptr_t> &dst, const std::vector<uintptr_t> &src)
{
    return {h.shard, h.which == 0 ? dst[(size_t)h.shard] : src[(size_t)h.shard]};
}

static void check_holds(const std::vector<uintptr_t> &dst, const std::vector<uintptr_t> &src, bool dst_exclusive)
{
    const std::vector<chandle::Hold> h = chandle::holds(dst, src, dst_exclusive);
    std::set<std::pair<int32_t, uintptr_t>> want;              // every distinct lock of the call, once
    for (size_t g = 0; g < dst.size(); ++g) {
        want.insert({(int32_t)g, dst[g]});
        if (!src.empty()) want.insert({(int32_t)g, src[g]});
    }
    CHECK(h.size() == want.size());
    std::set<std::pair<int32_t, uintptr_t>> seen;
    for (size_t i = 0; i < h.size(); ++i) {
        const auto k = key_of(h[i], dst, src);
        CHECK(want.count(k) == 1 && seen.insert(k).second);     // a lock of the call, not taken twice (src == dst: one hold)
        if (i > 0) CHECK(key_of(h[i - 1], dst, src) < k);        // strictly ascending in the one order: no cycle between two calls
        if (h[i].which == 0) CHECK(h[i].exclusive == (dst_exclusive || !src.empty()));   // what is written is held alone
        else CHECK(!h[i].exclusive && !src.empty());
    }
}

static void test_holds()
{
    {   // by hand: two shards, dst above src on shard 0 and below on shard 1
        const std::vector<chandle::Hold> h = chandle::holds({0x200, 0x300}, {0x100, 0x400}, true);
        CHECK(h == (std::vector<chandle::Hold>{{0, 1, false}, {0, 0, true}, {1, 0, true}, {1, 1, false}}));
        const std::vector<chandle::Hold> same = chandle::holds({0x200, 0x300}, {0x200, 0x300}, true);
        CHECK(same == (std::vector<chandle::Hold>{{0, 0, true}, {1, 0, true}}));
        const std::vector<chandle::Hold> rd = chandle::holds({0x200, 0x300, 0x50}, {}, false);
        CHECK(rd == (std::vector<chandle::Hold>{{0, 0, false}, {1, 0, false}, {2, 0, false}}));
    }
    std::mt19937_64 rng(5);
    for (int it = 0; it < 4000; ++it) {
        const size_t G = 1 + rng() % 5;
        std::vector<uintptr_t> dst(G), src(G);
        for (size_t g = 0; g < G; ++g) {
            dst[g] = 16 * (1 + rng() % 8);
            src[g] = rng() % 4 == 0 ? dst[g] : 16 * (1 + rng() % 8);
        }
        check_holds(dst, src, true);
        check_holds(dst, {}, true);
        check_holds(dst, {}, false);
        // two combines with the roles swapped take the locks they share in the same relative order
        const std::vector<chandle::Hold> ab = chandle::holds(dst, src, true), ba = chandle::holds(src, dst, true);
        std::vector<std::pair<int32_t, uintptr_t>> ka, kb;
        for (const chandle::Hold &x : ab) ka.push_back(key_of(x, dst, src));
        for (const chandle::Hold &x : ba) kb.push_back(key_of(x, src, dst));
        CHECK(ka == kb);
    }
}

// ---- the split from handle-reported counts -----------------------------------------------------------------------------------
// Brute force: every shard holds a list of rows with a flag "in the scope and live"; the counted lists give live[g] as the
// count step of the id-list call finds it, a handle reports the same number; ONE index over all rows lets the first
// max(1, limit) scoped live rows take part.
static void test_split()
{
    std::mt19937_64 rng(23);
    for (int it = 0; it < 3000; ++it) {
        const size_t G = 1 + rng() % 5;
        std::vector<std::vector<uint8_t>> rows(G);
        std::vector<int64_t> counted(G, 0), handle(G, 0);
        for (size_t g = 0; g < G; ++g) {
            rows[g].resize(rng() % 30);
            for (uint8_t &r : rows[g]) { r = rng() % 3 != 0; counted[g] += r; }
            handle[g] = (int64_t)std::count(rows[g].begin(), rows[g].end(), 1);     // what the handle keeps in `live`
        }
        for (int64_t limit : {(int64_t)-3, (int64_t)0, (int64_t)1, (int64_t)(rng() % 90), (int64_t)1000}) {
            const int64_t room = limit < 1 ? 1 : limit;
            std::vector<int64_t> before(G, 0), took(G, 0);
            int64_t seen = 0;
            for (size_t g = 0; g < G; ++g) {
                before[g] = seen;
                for (uint8_t r : rows[g]) {
                    if (!r) continue;
                    if (seen < room) ++took[g];
                    ++seen;
                }
            }
            cscope::Split s;
            CHECK(chandle::handle_split(handle, limit, s));
            const cscope::Split lists = cscope::split_limit(counted, limit);
            CHECK(s.before == before && s.took == took);
            CHECK(s.before == lists.before && s.took == lists.took && s.total == lists.total && s.largest == lists.largest);
            for (size_t g = 0; g < G; ++g)                      // what each shard's pass works out from scope_before alone
                CHECK(cscope::shard_took(handle[g], limit, s.before[g]) == took[g]);
        }
        // an orphaned part reports -1: nothing is split
        std::vector<int64_t> broken = handle;
        broken[rng() % G] = -1;
        cscope::Split keep;
        keep.total = 77;
        CHECK(!chandle::handle_split(broken, 10, keep) && keep.total == 77);
    }
    cscope::Split s;
    CHECK(chandle::handle_split({}, 5, s) && s.total == 0);
    CHECK(chandle::handle_split({0, 0, 0}, 5, s) && s.total == 0 && s.largest == 0);
}

int main()
{
    test_row_ids();
    test_pair();
    test_holds();
    test_split();
    if (g_failed) { printf("orr_cluster_handle_plan_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("orr_cluster_handle_plan_selftest: ok\n");
    return 0;
}
