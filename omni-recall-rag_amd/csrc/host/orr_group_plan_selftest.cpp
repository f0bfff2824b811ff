// orr_group_plan_selftest -- the rules of orr_group_plan.h on the CPU (no HIP, no GPU): the argument checks, a group's sample
// size with its two terms and its cap, the split into screen and list groups, the summed cost rule on both sides of its
// threshold under every mask_screen, the one-used-group shortcut, the ladder's next step and its bound, the workspace slice.
// Exit status 0 and a last line "orr_group_plan_selftest: ok" when everything holds; tests/test_group_plan_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../orr_group_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

using group::GroupIn;
using group::Plan;
using group::Role;

static void test_arguments()
{
    CHECK(group::kMaxGroups == 64);
    CHECK(!group::groups_valid(0) && group::groups_valid(1) && group::groups_valid(64) && !group::groups_valid(65) && !group::groups_valid(-1));
    const int32_t qg[] = {0, 2, 1, 2};
    CHECK(group::assignment_valid(qg, 4, 3));
    CHECK(!group::assignment_valid(qg, 4, 2));                      // group 2 of 2
    CHECK(!group::assignment_valid(nullptr, 4, 3));
    const int32_t neg[] = {0, -1};
    CHECK(!group::assignment_valid(neg, 2, 3));
    CHECK(group::took_of(100, 0) == 1 && group::took_of(100, 30) == 30 && group::took_of(20, 30) == 20 && group::took_of(0, 30) == 0);
    // the offsets of the groups are the scoped search's offsets with G pseudo-queries
    const uint64_t off[] = {0, 3, 3, 7};
    CHECK(scope::offsets_valid(off, 3, 7) && !scope::offsets_valid(off, 3, 8) && !scope::offsets_valid(off, 2, 7));
}

static void test_sample()
{
    // the first term by hand (orr_mask_plan.h's sample_rows): sqrt(k took) in whole lists, at least 256
    CHECK(mask::sample_rows(10, 20000) == 448 && mask::sample_rows(10, 100000) == 1024);
    CHECK(mask::sample_rows(10, 10000) == 320 && mask::sample_rows(10, 200) == 256);
    // with little in the other groups it decides
    CHECK(group::sample_rows(10, 20000, 100000, 8192) == 448);
    CHECK(group::sample_rows(10, 100000, 100000, 8192) == 1024);
    CHECK(group::sample_rows(10, 10000, 100000, 8192) == 320);
    CHECK(group::sample_rows(10, 200, 100000, 8192) == 256);       // (the buffer term: 2 x 10 x 100,000 / 8192 = 244.1 -> 245 -> 256)
    // the GPU test's groups sum to 130,200 rows: 317.9 -> 318 -> 320 lifts the smallest group's sample and no other
    CHECK(group::sample_rows(10, 200, 130200, 8192) == 320 && group::sample_rows(10, 10000, 130200, 8192) == 320);
    CHECK(group::sample_rows(10, 20000, 130200, 8192) == 448 && group::sample_rows(10, 100000, 130200, 8192) == 1024);
    // the buffer term takes over: 2 x 10 x 1,000,000 / 8192 = 2441.4 -> 2,442 -> whole lists: 2,496
    CHECK(group::sample_rows(10, 100000, 1000000, 8192) == 2496);
    CHECK(group::sample_rows(10, 200, 1000000, 8192) == 2496);      // ... for every group, so a small one becomes a list group
    CHECK(group::sample_rows(10, 100000, 1000000, 16384) == 1280);   // 1220.7 -> 1221 -> 1280: larger buffers, smaller sample
    CHECK(group::sample_rows(10, 100000, 800000, 16384) == 1024);    // 976.6 -> 977 -> 1024: the first term again
    // the cap
    CHECK(group::sample_rows(64, 1ll << 40, 1ll << 41, 8192) == 65536);
    CHECK(group::sample_rows(10, 100000, 1ll << 40, 8192) == 65536);
    for (int32_t k : {0, 1, 10, 64})
        for (int64_t sum : {1000ll, 1000000ll, 100000000ll}) {
            const int64_t m = group::sample_rows(k, 1000, sum, 8192);
            CHECK(m % 64 == 0 && m >= mask::sample_rows(k, 1000) && m <= mask::kMaxSampleRows);
            // what the rule is for: k sum / m pairs stay within half a buffer, unless the cap holds m down
            if (m < mask::kMaxSampleRows) CHECK(std::max(1, k) * sum / m <= 4096);
        }
    // the survivors' buffers of a pass, as select_fused halves them
    CHECK(group::pass_cap(8192, 256) == 8192 && group::pass_cap(8192, 100000) == 8192);
    CHECK(group::pass_cap(65536, 256) == 65536);                     // 256 x 65536 x 40 = 640 MiB
    CHECK(group::pass_cap(262144, 256) == 131072);                   // 2.5 GiB -> 1.25 GiB
}

static std::vector<GroupIn> issue_groups(int64_t limit)
{
    // the GPU test's groups on 200,000 rows: A 100,000, B 20,000, C 10,000, D 200, E empty, F named by no query
    const int64_t live[] = {100000, 20000, 10000, 200, 0, 5000};
    const int64_t last[] = {200000, 199990, 150000, 199000, 0, 120000};      // one past the group's last row
    const int32_t nq[] = {8, 8, 8, 8, 8, 0};
    std::vector<GroupIn> g(6);
    for (int i = 0; i < 6; ++i) {
        g[i].took = group::took_of(live[i], limit);
        g[i].n_clip = g[i].took == live[i] ? last[i] : last[i] * g[i].took / std::max<int64_t>(live[i], 1);
        g[i].queries = nq[i];
    }
    return g;
}

static void test_split()
{
    const std::vector<GroupIn> g = issue_groups(1000000);
    const Plan p = group::plan(g, 10, 8192, 1, true, 128, 64, 1);
    CHECK(p.used == 4 && p.only == -1 && p.sum_took == 130200);
    CHECK(p.role[0] == Role::Screen && p.role[1] == Role::Screen && p.role[2] == Role::Screen);
    CHECK(p.role[3] == Role::List);                                  // 200 rows <= its sample
    CHECK(p.role[4] == Role::Unused && p.role[5] == Role::Unused);   // empty; named by no query
    CHECK(p.sample[0] == 1024 && p.sample[1] == 448 && p.sample[2] == 320 && p.sample[3] == 320 && p.sample[4] == 0 && p.sample[5] == 0);
    CHECK(p.screen_groups == 3 && p.n_clip == 200000 && p.max_sample == 1024 && p.min_sample == 320 && p.min_took == 10000);
    CHECK(p.eligible && p.grouped);
    // a clip below what a two-stage pass needs: not eligible, whatever mask_screen says
    const std::vector<GroupIn> c = issue_groups(15000);
    CHECK(c[0].took == 15000 && c[1].took == 15000 && c[2].took == 10000);
    for (int ms : {0, 1, 2}) {
        const Plan q = group::plan(c, 10, 8192, ms, true, 128, 64, 1);
        CHECK(q.screen_groups == 3 && q.n_clip < mask::kMinScreenRows && !q.eligible && !q.grouped);
    }
    // what a two-stage pass needs besides the rows
    CHECK(!group::plan(g, 10, 8192, 1, false, 128, 64, 1).grouped);  // no cosine part
    CHECK(!group::plan(g, 10, 8192, 1, true, 100, 64, 1).grouped);   // dim % 64
    CHECK(!group::plan(g, 65, 8192, 1, true, 128, 64, 1).grouped);   // topk beyond a selection list
    CHECK(!group::plan(g, 10, 8192, 1, true, 128, 64, 0).grouped);   // two_stage off
    // only list groups: nothing to screen
    std::vector<GroupIn> small(3);
    for (auto &s : small) { s.took = 200; s.n_clip = 200000; s.queries = 4; }
    const Plan ps = group::plan(small, 10, 8192, 1, true, 128, 64, 1);
    CHECK(ps.used == 3 && ps.screen_groups == 0 && !ps.eligible && !ps.grouped);
    // the floor's selection may read only the lists' heads when EVERY query has 8 k lists
    CHECK(!group::floor_from_heads(320, 10, 64) && !group::floor_from_heads(5056, 10, 64) && group::floor_from_heads(5120, 10, 64));
    CHECK(group::floor_from_heads(512, 0, 64) && !group::floor_from_heads(448, 1, 64));
}

static void test_one_used_group()
{
    std::vector<GroupIn> g(3);
    g[0] = GroupIn{0, 0, 5};             // empty
    g[1] = GroupIn{50000, 900000, 7};    // the one used group
    g[2] = GroupIn{80000, 900000, 0};    // named by no query
    const Plan p = group::plan(g, 10, 8192, 1, true, 128, 64, 1);
    CHECK(p.used == 1 && p.only == 1 && !p.grouped && p.screen_groups == 0);
    CHECK(p.role[1] == Role::Unused);    // nothing of the plan runs: the masked call itself
    g[1].queries = 0;
    const Plan none = group::plan(g, 10, 8192, 1, true, 128, 64, 1);
    CHECK(none.used == 0 && none.only == -1 && !none.grouped);
    const Plan one = group::plan(std::vector<GroupIn>(1, GroupIn{50000, 900000, 7}), 10, 8192, 1, true, 128, 64, 1);
    CHECK(one.used == 1 && one.only == 0 && !one.grouped);
}

static void test_cost_rule()
{
    // two groups of 8 queries: max(4 x 8, 128) = 128 screened rows per scoped row; n_clip = 4,000,000 -> 31,250 rows in all
    auto two = [](int64_t t0, int64_t t1, int32_t q0, int32_t q1) {
        std::vector<GroupIn> g(2);
        g[0] = GroupIn{t0, 4000000, q0};
        g[1] = GroupIn{t1, 3900000, q1};
        return g;
    };
    CHECK(group::plan(two(15625, 15625, 8, 8), 10, 8192, 0, true, 128, 64, 1).grouped);     // 128 x 31,250 = 4,000,000
    CHECK(!group::plan(two(15625, 15624, 8, 8), 10, 8192, 0, true, 128, 64, 1).grouped);    // 128 x 31,249 = 3,999,872
    CHECK(group::plan(two(15625, 15624, 8, 8), 10, 8192, 1, true, 128, 64, 1).grouped);     // forced
    CHECK(!group::plan(two(15625, 15625, 8, 8), 10, 8192, 2, true, 128, 64, 1).grouped);    // forbidden
    CHECK(group::plan(two(15625, 15625, 8, 8), 10, 8192, 2, true, 128, 64, 1).eligible);
    // from 32 queries of a group on its factor is 4 B_g: 4 x 128 x 2,000 + 128 x 23,250 = 4,000,000
    CHECK(group::plan(two(2000, 23250, 128, 8), 10, 8192, 0, true, 128, 64, 1).grouped);
    CHECK(!group::plan(two(2000, 23249, 128, 8), 10, 8192, 0, true, 128, 64, 1).grouped);
    // a list group's rows do not count: only what the grouped pass would replace
    {
        std::vector<GroupIn> g = two(31249, 256, 8, 8);
        const Plan p = group::plan(g, 10, 8192, 0, true, 128, 64, 1);
        CHECK(p.role[0] == Role::Screen && p.role[1] == Role::List && !p.grouped);           // 128 x 31,249 < 4,000,000
        g[0].took = 31250;
        CHECK(group::plan(g, 10, 8192, 0, true, 128, 64, 1).grouped);
    }
    // a call of its own counts as at least 2^19 screened rows: two small groups pay on a shard of 1,000,000 rows (measured),
    // and on both sides of 2 x 524,288
    CHECK(group::kMinCallRows == 524288);
    {
        std::vector<GroupIn> s(2, GroupIn{3000, 1000000, 4});                                // 128 x 3,000 = 384,000 each
        CHECK(group::plan(s, 10, 8192, 0, true, 3072, 64, 1).grouped);
        s[0].n_clip = s[1].n_clip = 1048576;
        CHECK(group::plan(s, 10, 8192, 0, true, 3072, 64, 1).grouped);
        s[0].n_clip = 1048577;
        CHECK(!group::plan(s, 10, 8192, 0, true, 3072, 64, 1).grouped);
        s[0].took = 4097;                                                                    // 128 x 4,097 = 524,416: one row over the floor
        CHECK(group::plan(s, 10, 8192, 0, true, 3072, 64, 1).grouped);
    }
    // the measured cells (1M x 3072): the grouped pass won in all twelve, and the rule takes it in all twelve
    for (int32_t B : {8, 256})
        for (int32_t G : {2, 8})
            for (int64_t S : {3000ll, 30000ll, 100000ll})
                CHECK(group::plan(std::vector<GroupIn>((size_t)G, GroupIn{S, 1000000, B / G}), 10, 8192, 0, true, 3072, 64, 1).grouped);
    // ... but not on ten times the rows for two small groups
    CHECK(!group::plan(std::vector<GroupIn>(2, GroupIn{3000, 10000000, 4}), 10, 8192, 0, true, 3072, 64, 1).grouped);
    // no overflow in the sum
    {
        std::vector<GroupIn> g(64, GroupIn{(int64_t)1 << 40, (int64_t)1 << 61, 1 << 20});
        std::vector<Role> role(64, Role::Screen);
        CHECK(group::screen_pays(g, role, (int64_t)1 << 61));
        CHECK(!group::screen_pays(std::vector<GroupIn>(2, GroupIn{1, 2000000, 1}), std::vector<Role>(2, Role::Screen), 2000000));
    }
}

static void test_ladder()
{
    using group::Step;
    // an overflow larger buffers can hold: they grow once, to this call's own size
    group::Next n = group::next_step(true, false, 8192, 30000, 200000, 3);
    CHECK(n.step == Step::GrowBuffers && n.new_cap == 65536);        // 8192 doubled until it holds 30,000 + an eighth
    n = group::next_step(true, true, 65536, 70000, 200000, 3);       // grown already
    CHECK(n.step == Step::GroupLadder);
    n = group::next_step(false, false, 8192, 30000, 200000, 3);      // something else kept a query uncertified
    CHECK(n.step == Step::GroupLadder);
    n = group::next_step(true, false, 8192, 150000, 200000, 3);      // more than half the rows: buffers are not the answer
    CHECK(n.step == Step::GroupLadder);
    n = group::next_step(true, false, 8192, 1u << 19, (int64_t)1 << 30, 3);
    CHECK(n.step == Step::GroupLadder);
    // the bound: the pass, its one repeat, then the group's own ladder, which orr_mask_plan.h bounds
    int passes = 1;
    bool grown = false;
    for (;;) {
        const group::Next s = group::next_step(true, grown, 8192, 30000, 200000, 1);
        if (s.step != Step::GrowBuffers) break;
        grown = true;
        ++passes;
        CHECK(passes <= group::kMaxGroupedPasses);
    }
    CHECK(passes == group::kMaxGroupedPasses && group::kMaxGroupedPasses == 2);
    CHECK(group::kMaxPassesBeforeListParts == 2 + 1 + mask::kMaxScreenRepeats);
}

static void test_workspace()
{
    // as the masked call's slice, with the largest sample of the batch
    CHECK(group::screen_slice(256, 1024) == mask::screen_slice(256, 1024) && group::screen_slice(256, 1024) == 256);
    CHECK(group::screen_slice(100000, 1024) == (int32_t)(escalation::kPassWorkspaceBytes / (40 * 8192)));
    CHECK(group::screen_slice(100000, 65536) == (int32_t)(escalation::kPassWorkspaceBytes / (40 * 65536)));
    CHECK(group::screen_slice(0, 1024) == 1);
}

int main()
{
    test_arguments();
    test_sample();
    test_split();
    test_one_used_group();
    test_cost_rule();
    test_ladder();
    test_workspace();
    if (g_failed) { printf("orr_group_plan_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("orr_group_plan_selftest: ok\n");
    return 0;
}
