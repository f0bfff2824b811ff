// orr_cluster_scope_plan_selftest -- the rules of orr_cluster_scope_plan.h on the CPU (no HIP, no GPU): the split of the global
// candidate_limit over the shards against a row-by-row restatement, the ladder (monotone, ends where every scoped row is a
// record, within its stated bound) and the slices of a merge against a brute-force count.
// Exit status 0 and a last line "orr_cluster_scope_plan_selftest: ok" when everything holds;
// tests/test_cluster_scope_plan_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../orr_cluster_scope_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

// The split as ONE index over all rows makes it: walk the scoped live rows in the global order, let the first max(1, limit)
// take part, count them per shard.
static void brute_split(const std::vector<int64_t> &live, int64_t limit, std::vector<int64_t> &before, std::vector<int64_t> &took)
{
    const int64_t room = limit < 1 ? 1 : limit;
    before.assign(live.size(), 0);
    took.assign(live.size(), 0);
    int64_t seen = 0;
    for (size_t g = 0; g < live.size(); ++g) {
        before[g] = seen;
        for (int64_t r = 0; r < live[g]; ++r) {
            if (seen < room) ++took[g];
            ++seen;
        }
    }
}

static void check_split(const std::vector<int64_t> &live, int64_t limit)
{
    std::vector<int64_t> before, took;
    brute_split(live, limit, before, took);
    const cscope::Split s = cscope::split_limit(live, limit);
    CHECK(s.before == before);
    CHECK(s.took == took);
    int64_t total = 0, largest = 0, all = 0;
    for (size_t g = 0; g < live.size(); ++g) {
        total += took[g];
        largest = std::max(largest, took[g]);
        all += live[g];
        CHECK(cscope::shard_took(live[g], limit, before[g]) == took[g]);            // what a shard works out for itself
        CHECK(cscope::shard_limit(limit, before[g]) >= took[g]);
    }
    CHECK(s.total == total && s.largest == largest);
    CHECK(total == std::min<int64_t>(all, std::max<int64_t>(1, limit)));            // what one index lets take part
}

static void test_split()
{
    // by hand: three shards, the limit ends inside the second
    {
        const cscope::Split s = cscope::split_limit({100, 250, 80}, 300);
        CHECK(s.before == (std::vector<int64_t>{0, 100, 350}));
        CHECK(s.took == (std::vector<int64_t>{100, 200, 0}));
        CHECK(s.total == 300 && s.largest == 200);
    }
    CHECK(cscope::shard_limit(0, 0) == 1 && cscope::shard_limit(-5, 0) == 1 && cscope::shard_limit(0, 1) == 0);
    CHECK(cscope::shard_limit(10, -3) == 10);                                        // a negative `before` counts as none
    CHECK(cscope::shard_took(-1, 10, 0) == 0);
    std::mt19937_64 rng(7);
    for (int G = 1; G <= 64; ++G)
        for (int rep = 0; rep < 12; ++rep) {
            std::vector<int64_t> live((size_t)G);
            int64_t all = 0;
            for (auto &l : live) {
                const uint64_t r = rng();
                l = r % 4 == 0 ? 0 : (int64_t)(r >> 8) % 300;                        // shards without a scoped row among them
                all += l;
            }
            if (rep == 0) std::fill(live.begin(), live.end(), 0);                    // no scoped row anywhere
            const int64_t inside = live[(size_t)G / 2] > 1 ? all / 2 : 1;
            for (int64_t limit : {(int64_t)-3, (int64_t)0, (int64_t)1, (int64_t)2, live[0], live[0] + 1, inside, all - 1, all, all + 1, all * 3 + 7, INT64_MAX})
                check_split(live, limit);
        }
}

static void walk_ladder(bool masked, int32_t take, int64_t total, int64_t largest, int screen_for)
{
    const int32_t W = 64;
    cscope::Rung r = cscope::first_rung(masked, take, total, W);
    CHECK(r.kprime >= 1 && !r.done);
    CHECK(r.kprime == escalation::initial_kprime(take, total, W));
    CHECK(masked || r.pass == 0);
    int passes = 1;
    for (;;) {
        const bool screened = masked && r.pass == 0 && r.kprime <= W && passes <= screen_for;      // a shard can screen only at pass 0 within a list
        const cscope::Rung n = cscope::next_rung(r, masked, screened, largest, W);
        if (n.done) {
            // the end: the last pass was on the list path with every scoped row of every shard a record
            CHECK(r.kprime >= std::max<int64_t>(1, largest));
            CHECK(!screened);
            break;
        }
        CHECK(n.kprime >= r.kprime && n.pass >= r.pass);
        CHECK(n.kprime > r.kprime || n.pass > r.pass);                               // strictly more than before
        CHECK(n.pass == 0 || masked);
        CHECK(n.pass == 1 || n.kprime <= W || !masked);                              // a masked search beyond a list is on the list path
        if (n.kprime > r.kprime) CHECK(n.kprime == std::min<int64_t>(r.kprime * 4, std::max<int64_t>(1, largest)));
        if (screened && n.pass == 1) CHECK(n.kprime == r.kprime && (r.kprime * 4 > W || r.kprime >= largest));
        r = n;
        ++passes;
        if (passes > 200) { CHECK(!"the ladder does not end"); break; }
    }
    CHECK(passes <= cscope::ladder_bound(largest));
    CHECK(passes <= cscope::kMaxRungs);
}

static void test_ladder()
{
    for (bool masked : {false, true})
        for (int32_t take : {1, 5, 10, 40, 64, 100, 1000})
            for (int64_t largest : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)31, (int64_t)32, (int64_t)64, (int64_t)65, (int64_t)70, (int64_t)1000, (int64_t)20000,
                                    (int64_t)196608, (int64_t)4194240, (int64_t)1 << 31, (int64_t)1 << 40, INT64_MAX / 64})
                for (int64_t shards : {1, 2, 64})
                    for (int screen_for : {0, 1, 2, 100})
                        walk_ladder(masked, take, largest > INT64_MAX / 64 / shards ? largest : largest * shards, largest, screen_for);
    CHECK(cscope::ladder_bound(0) == 2 && cscope::ladder_bound(1) == 2 && cscope::ladder_bound(4) == 3 && cscope::ladder_bound(5) == 4);
    CHECK(cscope::ladder_bound(INT64_MAX) == cscope::kMaxRungs);
    // by hand: topk 10 over 70 equal rows on one shard of two -- 32 behind the screen, then the list, then all 70
    {
        cscope::Rung r = cscope::first_rung(true, 10, 20000, 64);
        CHECK(r.kprime == 32 && r.pass == 0);
        r = cscope::next_rung(r, true, true, 15000, 64);
        CHECK(r.kprime == 32 && r.pass == 1 && !r.done);                             // 128 fits no list
        r = cscope::next_rung(r, true, false, 15000, 64);
        CHECK(r.kprime == 128 && r.pass == 1);
        // no shard screened: the first pass was the list path already
        r = cscope::next_rung(cscope::first_rung(true, 10, 20000, 64), true, false, 15000, 64);
        CHECK(r.kprime == 128 && r.pass == 1);
        // topk 100: beyond a list from the start
        r = cscope::first_rung(true, 100, 20000, 64);
        CHECK(r.kprime == 122 && r.pass == 1);
        CHECK(cscope::first_rung(false, 100, 20000, 64).pass == 0);
    }
}

static void test_slices()
{
    const size_t budget = (size_t)1 << 30;
    for (int32_t nq : {1, 7, 256, 1024})
        for (int32_t shards : {1, 2, 8, 64})
            for (int64_t k : {(int64_t)1, (int64_t)32, (int64_t)64, (int64_t)1000, (int64_t)65536, (int64_t)4194240}) {
                const int32_t w = cscope::merge_slice(nq, shards, k, budget);
                CHECK(w >= 1 && w <= nq);
                const auto bytes = [&](int64_t q) { return (unsigned __int128)q * (unsigned __int128)shards * (unsigned __int128)(k + 1) * 56u; };
                CHECK(w == 1 || bytes(w) <= budget);                                 // within the budget, or one query alone
                CHECK(w == nq || bytes((int64_t)w + 1) > budget);                    // and no narrower than it has to be
                // every query lies in exactly one slice
                int32_t covered = 0;
                for (int32_t b0 = 0; b0 < nq; b0 += w) covered += std::min(w, nq - b0);
                CHECK(covered == nq);
            }
    CHECK(cscope::merge_slice(256, 2, 32, budget) == 256);
    CHECK(cscope::merge_slice(0, 0, 0, budget) == 1);
    CHECK(cscope::kRecordBytes == 56);
}

int main()
{
    test_split();
    test_ladder();
    test_slices();
    if (g_failed) { printf("orr_cluster_scope_plan_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("orr_cluster_scope_plan_selftest: ok\n");
    return 0;
}
