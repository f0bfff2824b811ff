// The escalation ladder (../orr_escalation.h) on the CPU: no HIP, no GPU.
//   orr_escalation_selftest <scenario>      exit status 0: the scenario held; 1: a check failed; 2: usage
// tests/test_escalation_cpu.py runs every scenario.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../orr_escalation.h"

namespace {

using namespace escalation;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); fflush(stderr); std::_Exit(1); } \
    } while (0)

constexpr int64_t kRows = 10'000'000;

// a shard whose two-stage pass (fused, on the matrix cores) kept `counts`
ShardOutcome screened(std::vector<uint32_t> counts, uint32_t pass_cap = 8192, uint32_t survivor_cap = 0, int64_t n = kRows)
{
    ShardOutcome o;
    o.two_stage = o.fused = o.use_mfma = true;
    o.pass_cap = pass_cap;
    o.survivor_cap = survivor_cap ? survivor_cap : pass_cap;
    o.n = n;
    o.survivors = std::move(counts);
    return o;
}

ShardOutcome plain(bool fused, bool use_mfma, int64_t n = kRows)      // a pass that kept no survivors
{
    ShardOutcome o;
    o.fused = fused; o.use_mfma = use_mfma; o.pass_cap = o.survivor_cap = 8192; o.n = n;
    return o;
}

void rungs_in_order()
{
    // overflow only: the same pass again, with the cap grown_survivor_cap gives
    uint32_t cap = 0;
    CHECK(grown_survivor_cap(8192, 20000, kRows, 1, &cap) && cap == 32768);
    Decision d = decide({screened({100, 20000, 5})}, {1, 0, 1}, false, false, 32, kRows, false);
    CHECK(d.step == Step::GrowBuffers && d.again == std::vector<int32_t>{1} && d.new_cap == std::vector<uint32_t>{32768} && d.kprime == 32);
    // a tie at the cut under a fused pass
    d = decide({screened({100, 200, 5}, 32768)}, {1, 0, 0}, false, false, 32, kRows, false);
    CHECK(d.step == Step::Unfused && (d.again == std::vector<int32_t>{1, 2}) && d.new_cap.empty());
    // then the unfused pass (still on the matrix cores), then the exact one, then k' x 4, capped by the rows
    d = decide({plain(false, true)}, {0}, true, false, 32, kRows, false);
    CHECK(d.step == Step::Exact && d.again == std::vector<int32_t>{0} && d.kprime == 32);
    d = decide({plain(false, false)}, {0}, true, true, 32, kRows, false);
    CHECK(d.step == Step::WiderK && d.kprime == 128 && d.again == std::vector<int32_t>{0});
    d = decide({plain(false, false, 100)}, {0}, true, true, 32, 100, false);
    CHECK(d.step == Step::WiderK && d.kprime == 100);
    d = decide({plain(false, false, 100)}, {0}, true, true, 100, 100, false);
    CHECK(d.step == Step::Exhausted && d.again.empty());
    d = decide({screened({100, 20000, 5})}, {1, 1, 1}, false, false, 32, kRows, false);
    CHECK(d.step == Step::Done && d.again.empty() && d.kprime == 32);
}

void mixed_causes()
{
    // one uncertified query overflowed, another did not: larger buffers do not help the second
    Decision d = decide({screened({20000, 200})}, {0, 0}, false, false, 32, kRows, false);
    CHECK(d.step == Step::Unfused && (d.again == std::vector<int32_t>{0, 1}));
    d = decide({screened({20000, 200})}, {0, 0}, false, false, 32, kRows, true);
    CHECK(d.step == Step::Unfused);
    // the certified query's overflow does not count, the uncertified one's does
    d = decide({screened({20000, 9000})}, {1, 0}, false, false, 32, kRows, false);
    CHECK(d.step == Step::GrowBuffers && d.new_cap == std::vector<uint32_t>{16384});
}

void growth_refused()
{
    uint32_t cap = 0;
    CHECK(!grown_survivor_cap(8192, 1u << 19, kRows, 1, &cap));
    CHECK(grown_survivor_cap(8192, (1u << 19) - 1, kRows, 1, &cap) && cap == (1u << 20));
    CHECK(!grown_survivor_cap(8192, 10000, 20000, 1, &cap) && grown_survivor_cap(8192, 10000, 20001, 1, &cap));
    CHECK(!grown_survivor_cap(8192, 22370, kRows, 1000, &cap));       // 1000 x 22370 x 96 B >= 2 GiB
    CHECK(grown_survivor_cap(8192, 22369, kRows, 1000, &cap));
    // each of them: the next rung instead
    CHECK(decide({screened({1u << 19})}, {0}, false, false, 32, kRows, false).step == Step::Unfused);
    CHECK(decide({screened({10000}, 8192, 0, 20000)}, {0}, false, false, 32, 20000, false).step == Step::Unfused);
    std::vector<uint32_t> many(1000, 22370);
    CHECK(decide({screened(many)}, std::vector<uint8_t>(1000, 0), false, false, 32, kRows, false).step == Step::Unfused);
    many.assign(1000, 22369);
    CHECK(decide({screened(many)}, std::vector<uint8_t>(1000, 0), false, false, 32, kRows, false).step == Step::GrowBuffers);
}

void three_shards()
{
    // overflow on one shard only: that shard grows, the others are left alone
    Decision d = decide({screened({10, 20}), screened({30, 20000}), screened({5, 6})}, {1, 0}, false, false, 32, 3 * kRows, true);
    CHECK(d.step == Step::GrowBuffers && (d.new_cap == std::vector<uint32_t>{0, 32768, 0}) && d.again == std::vector<int32_t>{1});
    // two uncertified queries, each over on another shard
    d = decide({screened({9000, 20}), screened({30, 20000}), screened({5, 6})}, {0, 0}, false, false, 32, 3 * kRows, true);
    CHECK(d.step == Step::GrowBuffers && (d.new_cap == std::vector<uint32_t>{16384, 32768, 0}));
    // growth possible on one shard and refused on another (too few rows there): a more exact pass for all of them
    d = decide({screened({9000, 20}), screened({30, 20000}, 8192, 0, 30000), screened({5, 6})}, {0, 0}, false, false, 32, 2 * kRows, true);
    CHECK(d.step == Step::Unfused && d.new_cap.empty() && (d.again == std::vector<int32_t>{0, 1}));
    // a shard whose pass was not two-stage (a small shard: exact kernel) says nothing about its survivors
    d = decide({screened({10, 20000}), plain(false, false, 1000), screened({5, 6})}, {1, 0}, false, false, 32, 2 * kRows, true);
    CHECK(d.step == Step::Unfused);
    d = decide({plain(false, true), plain(false, false, 1000), plain(false, false)}, {1, 0}, true, false, 32, 2 * kRows, true);
    CHECK(d.step == Step::Exact);                     // one shard on the matrix cores is enough
}

void repeat_only_if_grown()
{
    // a large batch ran with halved buffers (pass_cap < survivor_cap); the cap the counts ask for is not above survivor_cap
    const ShardOutcome halved = screened({9000}, 8192, 16384);
    Decision d = decide({halved}, {0}, false, false, 32, kRows, false);
    CHECK(d.step == Step::GrowBuffers && d.new_cap == std::vector<uint32_t>{16384});      // one index: the sub-batch repeats the pass
    d = decide({halved}, {0}, false, false, 32, kRows, true);
    CHECK(d.step == Step::Unfused);                                                        // cluster: the next rung
    // where the cap rises above survivor_cap the flag makes no difference
    for (bool flag : {false, true}) {
        d = decide({screened({20000}, 8192, 16384)}, {0}, false, false, 32, kRows, flag);
        CHECK(d.step == Step::GrowBuffers && d.new_cap == std::vector<uint32_t>{32768});
    }
    // several shards: one raised cap is enough
    d = decide({halved, screened({20000}, 8192, 16384)}, {0}, false, false, 32, 2 * kRows, true);
    CHECK(d.step == Step::GrowBuffers && (d.new_cap == std::vector<uint32_t>{16384, 32768}));
    d = decide({halved, halved}, {0}, false, false, 32, 2 * kRows, true);
    CHECK(d.step == Step::Unfused);
}

// Feeds decide() "still uncertified" until the ladder ends.  The plan is as free as plan_pass' invariants leave it; after
// GrowBuffers the repeat runs with at least the cap decided (the header says why).  hostile: every screen overflows again by one.
int ladder_length(bool fused0, bool two_stage0, bool mfma0, bool no_fuse, bool force_exact, int64_t n, int64_t kprime, uint32_t worst,
                  bool only_if_grown, bool hostile)
{
    uint32_t pass_cap = 8192, survivor_cap = 8192;
    for (int repeats = 0;; ++repeats) {
        CHECK(repeats <= kMaxRepeats);
        ShardOutcome o;
        o.fused = fused0 && !no_fuse;
        o.two_stage = two_stage0 && o.fused;
        o.use_mfma = mfma0 && !force_exact;
        o.pass_cap = pass_cap; o.survivor_cap = survivor_cap; o.n = n;
        if (o.two_stage) o.survivors.assign(1, hostile ? pass_cap + 1 : worst);
        const Decision d = decide({o}, {0}, no_fuse, force_exact, kprime, n, only_if_grown);
        switch (d.step) {
        case Step::Done: CHECK(false); break;
        case Step::Exhausted: CHECK(kprime >= n); return repeats;
        case Step::GrowBuffers:
            CHECK(d.new_cap[0] > pass_cap);
            survivor_cap = std::max(survivor_cap, d.new_cap[0]);
            pass_cap = std::max(pass_cap, d.new_cap[0]);
            break;
        case Step::Unfused: CHECK(!no_fuse); no_fuse = true; break;
        case Step::Exact: CHECK(!force_exact); force_exact = true; break;
        case Step::WiderK: CHECK(d.kprime > kprime && d.kprime <= n); kprime = d.kprime; break;
        }
    }
}

void termination()
{
    int longest = 0;
    for (int bits = 0; bits < 128; ++bits)
        for (int64_t n : {(int64_t)1, (int64_t)33, (int64_t)100000, kRows, (int64_t)1 << 40, (int64_t)1 << 61})
            for (int64_t kprime : {(int64_t)1, (int64_t)32, (int64_t)64, (int64_t)4096})
                for (uint32_t worst : {0u, 8192u, 8193u, 40000u, (1u << 19) - 1, 1u << 19, 600000u}) {
                    if (kprime > n) continue;
                    const int len = ladder_length(bits & 1, bits & 2, bits & 4, bits & 8, bits & 16, n, kprime, worst, bits & 32, bits & 64);
                    longest = std::max(longest, len);
                }
    CHECK(longest > 6 + 1 + 1 && longest <= kMaxRepeats);             // (the grid does reach every kind of rung)
    // the longest ladder there is: six growths, both flags, k' from 1 to 2^61
    CHECK(ladder_length(true, true, true, false, false, (int64_t)1 << 61, 1, 0, false, true) == kMaxRepeats);
}

// ---- the decision parts of search_ids and cluster_search_ids as they were before escalate() replaced them: the launches, the
// statistics and the recursion cut away, the lines that decide kept as they stood.  (This scenario is the proof that decide()
// took both over; once that is history it may go.)
struct OldLane {
    std::vector<uint32_t> h_survivors;
    uint32_t pass_cap, survivor_cap;
    int64_t n;                                        // participating_rows(lane, candidate_limit)
};
struct OldPass {
    bool two_stage_, fused_, use_mfma;
    bool two_stage() const { return two_stage_; }
    bool fused() const { return fused_; }
};
struct OldDecision {
    Step step;
    std::vector<int32_t> again;
    int64_t kprime;
};

OldDecision old_index_decision(OldLane *idx, const OldPass &pass, const std::vector<uint8_t> &cert, bool cur_no_fuse, int64_t kprime, int64_t n)
{
    const int32_t nb = (int32_t)cert.size();
    int32_t unc = 0;
    for (uint8_t c : cert) unc += !c;
    uint32_t worst_unc_survivors = 0;
    bool unc_only_overflow = unc > 0;
    if (pass.two_stage() && (int32_t)idx->h_survivors.size() == nb) {
        for (int32_t i = 0; i < nb; ++i) {
            const uint32_t c = idx->h_survivors[(size_t)i];
            if (!cert[(size_t)i]) {
                if (c > idx->pass_cap) worst_unc_survivors = std::max(worst_unc_survivors, c);
                else unc_only_overflow = false;
            }
        }
    } else {
        unc_only_overflow = false;
    }
    if (unc == 0) return {Step::Done, {}, kprime};

    std::vector<int32_t> again;
    for (int32_t i = 0; i < nb; ++i) if (!cert[(size_t)i]) again.push_back(i);
    uint32_t cap = 0;
    if (unc_only_overflow && grown_survivor_cap(idx->pass_cap, worst_unc_survivors, n, again.size(), &cap)) {
        if (cap > idx->survivor_cap) idx->survivor_cap = cap;
        return {Step::GrowBuffers, again, kprime};
    } else if (pass.fused() && !cur_no_fuse) {
        return {Step::Unfused, again, kprime};
    } else if (pass.use_mfma) {
        return {Step::Exact, again, kprime};
    } else if (kprime >= n) {
        return {Step::Exhausted, {}, kprime};
    } else {
        kprime = std::min<int64_t>(n, kprime * 4);
    }
    return {Step::WiderK, again, kprime};
}

OldDecision old_cluster_decision(const std::vector<OldLane *> &on, const std::vector<uint8_t> &used_two_stage, const std::vector<uint8_t> &used_fused,
                                 const std::vector<uint8_t> &used_mfma, const std::vector<uint8_t> &cert, bool orig_no_fuse,
                                 bool orig_force_exact, int64_t kprime, int64_t n_total)
{
    const int32_t nb = (int32_t)cert.size(), G = (int32_t)on.size();
    int32_t unc = 0;
    for (uint8_t c : cert) unc += !c;
    bool any_fused = false, any_mfma = false, grow = false, only_overflow = unc > 0;
    for (int32_t g = 0; g < G; ++g) {
        OldLane *sh = on[(size_t)g];
        any_fused = any_fused || used_fused[(size_t)g];
        any_mfma = any_mfma || used_mfma[(size_t)g];
        if (!used_two_stage[(size_t)g] || (int32_t)sh->h_survivors.size() != nb) continue;
        uint32_t worst = 0;
        for (int32_t i = 0; i < nb; ++i) {
            const uint32_t cnt = sh->h_survivors[(size_t)i];
            if (cnt > sh->pass_cap) { if (!cert[(size_t)i]) worst = std::max(worst, cnt); }
        }
        uint32_t cap = 0;
        if (worst > 0 && grown_survivor_cap(sh->pass_cap, worst, sh->n, (size_t)unc, &cap)) {
            if (cap > sh->survivor_cap) { sh->survivor_cap = cap; grow = true; }
        } else if (worst > 0) {
            only_overflow = false;                                          // too many survivors to buffer: a more exact pass instead
        }
    }
    if (unc == 0) return {Step::Done, {}, kprime};
    // queries uncertified for a reason other than an overflowing buffer need a more exact pass whatever the buffers do
    if (grow) {
        for (int32_t g = 0; g < G && only_overflow; ++g) {
            OldLane *sh = on[(size_t)g];
            if (!used_two_stage[(size_t)g] || (int32_t)sh->h_survivors.size() != nb) { only_overflow = false; break; }
        }
        if (only_overflow)
            for (int32_t i = 0; i < nb && only_overflow; ++i) {
                if (cert[(size_t)i]) continue;
                bool over = false;
                for (int32_t g = 0; g < G; ++g) over = over || on[(size_t)g]->h_survivors[(size_t)i] > on[(size_t)g]->pass_cap;
                only_overflow = over;
            }
    }
    std::vector<int32_t> again;
    for (int32_t i = 0; i < nb; ++i) if (!cert[(size_t)i]) again.push_back(i);
    if (grow && only_overflow) {
        return {Step::GrowBuffers, again, kprime};
    } else if (any_fused && !orig_no_fuse) {
        return {Step::Unfused, again, kprime};
    } else if (any_mfma && !orig_force_exact) {
        return {Step::Exact, again, kprime};
    } else if (kprime >= n_total) {
        return {Step::Exhausted, {}, kprime};
    } else {
        kprime = std::min<int64_t>(n_total, kprime * 4);
    }
    return {Step::WiderK, again, kprime};
}

// what one shard's pass can leave behind: every plan plan_pass can make, caps, counts around pass_cap
struct ShardCase { OldPass pass; uint32_t pass_cap, survivor_cap; std::vector<uint32_t> counts; int64_t n; };

// (G = 1: all of them; more shards: fewer values each, so that the product stays small)
std::vector<ShardCase> shard_cases(int nb, int G)
{
    const OldPass plans[] = {{false, false, false}, {false, true, true}, {true, true, true}, {false, false, true}, {false, true, false}, {true, true, false}};
    std::vector<ShardCase> out;
    for (int p = 0; p < (G == 3 ? 3 : 6); ++p)
        for (uint32_t pass_cap : {8192u, 32768u})
            for (uint32_t mult : {1u, 2u, 8u})
                for (int64_t n : {(int64_t)60000, kRows}) {
                    const OldPass &plan = plans[p];
                    if (G > 1 && (mult == 2 || pass_cap == 32768 || (n != kRows && !plan.two_stage_))) continue;
                    if (G == 3 && nb == 3 && n != kRows) continue;
                    const uint32_t levels[] = {0, pass_cap, pass_cap + 1, 600000};
                    const int n_counts = plan.two_stage_ ? 1 << (2 * nb) : 1;     // (only a two-stage pass keeps counts)
                    for (int code = 0; code < n_counts; ++code) {
                        ShardCase c{plan, pass_cap, pass_cap * mult, {}, n};
                        bool zero = false;
                        for (int i = 0; i < nb && plan.two_stage_; ++i) {
                            c.counts.push_back(levels[(code >> (2 * i)) & 3]);
                            zero = zero || c.counts.back() == 0;
                        }
                        if (!(G == 3 && nb == 3 && zero)) out.push_back(c);
                    }
                }
    return out;
}

long compare_all(int G, int nb, long *index_and_cluster_differ)
{
    const std::vector<ShardCase> cases = shard_cases(nb, G);
    std::vector<size_t> pick((size_t)G, 0);
    long compared = 0;
    for (;;) {
        bool any_fused = false, any_mfma = false;
        int64_t n_total = 0;
        std::vector<ShardOutcome> shards;
        std::vector<OldLane> lanes;
        std::vector<OldLane *> on;
        std::vector<uint8_t> ts, fu, mf;
        for (size_t g : pick) {
            const ShardCase &c = cases[g];
            any_fused |= c.pass.fused_; any_mfma |= c.pass.use_mfma; n_total += c.n;
            ShardOutcome o;
            o.two_stage = c.pass.two_stage_; o.fused = c.pass.fused_; o.use_mfma = c.pass.use_mfma;
            o.pass_cap = c.pass_cap; o.survivor_cap = c.survivor_cap; o.n = c.n; o.survivors = c.counts;
            shards.push_back(o);
            lanes.push_back(OldLane{c.counts, c.pass_cap, c.survivor_cap, c.n});
            ts.push_back(c.pass.two_stage_); fu.push_back(c.pass.fused_); mf.push_back(c.pass.use_mfma);
        }
        for (OldLane &l : lanes) on.push_back(&l);
        // a decision of decide() against an old one, and against the caps the old code left on its lanes (which are then put back).
        // (The old cluster code also raised a shard's cap when it went on to another rung; decide() does so with GrowBuffers only.)
        auto same = [&](const Decision &d, const OldDecision &old) {
            bool ok = d.step == old.step && d.again == old.again && d.kprime == old.kprime;
            for (size_t g = 0; g < lanes.size(); ++g) {
                if (d.step == Step::GrowBuffers && std::max(shards[g].survivor_cap, d.new_cap[g]) != lanes[g].survivor_cap) ok = false;
                lanes[g].survivor_cap = shards[g].survivor_cap;
            }
            return ok;
        };
        for (int flags = 0; flags < 4; ++flags) {
            const bool no_fuse = flags & 1, force_exact = flags & 2;
            if ((no_fuse && any_fused) || (force_exact && any_mfma)) continue;          // plan_pass makes no such plan
            for (int certs = 0; certs < 1 << nb; ++certs)
                for (int64_t kprime : {(int64_t)32, n_total}) {
                    std::vector<uint8_t> cert;
                    for (int i = 0; i < nb; ++i) cert.push_back((certs >> i) & 1);
                    const OldDecision old_cluster = old_cluster_decision(on, ts, fu, mf, cert, no_fuse, force_exact, kprime, n_total);
                    CHECK(same(decide(shards, cert, no_fuse, force_exact, kprime, n_total, true), old_cluster));
                    ++compared;
                    if (G > 1) continue;
                    const OldDecision old_index = old_index_decision(&lanes[0], cases[pick[0]].pass, cert, no_fuse, kprime, n_total);
                    const Decision d = decide(shards, cert, no_fuse, force_exact, kprime, n_total, false);
                    CHECK(same(d, old_index));
                    // the two old functions differ in one way only: the repeat with a cap that is not above survivor_cap
                    if (old_index.step != old_cluster.step) {
                        ++*index_and_cluster_differ;
                        CHECK(old_index.step == Step::GrowBuffers && d.new_cap[0] <= shards[0].survivor_cap && old_cluster.step != Step::GrowBuffers);
                    } else {
                        CHECK(old_index.again == old_cluster.again && old_index.kprime == old_cluster.kprime);
                    }
                }
        }
        size_t g = 0;
        while (g < pick.size() && ++pick[g] == cases.size()) pick[g++] = 0;
        if (g == pick.size()) return compared;
    }
}

void old_against_new()
{
    long compared = 0, differ = 0;
    for (int G = 1; G <= 3; ++G)
        for (int nb = 1; nb <= 3; ++nb) compared += compare_all(G, nb, &differ);
    CHECK(compared > 1000000 && differ > 0);
    fprintf(stderr, "%ld inputs compared; the two old functions differ on %ld of the one-shard ones\n", compared, differ);
}

void survivors_accounted()
{
    orr_search_stats s{};
    s.survivors_max = 50; s.survivor_capacity = 16384;
    account_survivors(s, screened({10, 9000, 8192, 70}, 8192, 8192), 4);
    CHECK(s.survivors_total == 17272 && s.survivor_samples == 4 && s.survivors_max == 9000 && s.overflowed_queries == 1 && s.survivor_capacity == 16384);
    account_survivors(s, screened({40000, 3}, 32768, 65536), 2);
    CHECK(s.survivors_total == 57275 && s.survivor_samples == 6 && s.survivors_max == 40000 && s.overflowed_queries == 2 && s.survivor_capacity == 65536);
    const orr_search_stats before = s;
    account_survivors(s, plain(true, true), 2);                       // no two-stage pass: no counts
    account_survivors(s, screened({1, 2, 3}), 2);                     // counts of another batch
    CHECK(memcmp(&s, &before, sizeof(s)) == 0);
    CHECK(s.passes == 0 && s.requeried == 0 && s.buffer_growths == 0);
}

void slices_and_first_kprime()
{
    const int64_t n = 1 << 20;                                        // 8 MiB per query: 512 queries fill kPassWorkspaceBytes
    CHECK(kPassWorkspaceBytes == (size_t)4 << 30);
    CHECK(slice_width(512, n, true) == 0 && slice_width(513, n, true) == 512 && slice_width(100000, n, true) == 512);
    CHECK(slice_width(100000, n, false) == 0);                        // the fused passes keep nothing per (query,row)
    CHECK(slice_width(513, n + 1, true) == 511);
    CHECK(slice_width(1, (int64_t)1 << 40, true) == 0 && slice_width(2, (int64_t)1 << 40, true) == 1);      // one query is never cut
    CHECK(slice_width(1 << 30, 0, true) == 1 << 29);                  // an empty shard counts as one row
    // every slice then goes in one piece
    for (int32_t nb : {2, 513, 4097}) {
        const int32_t per = slice_width(nb, n + 12345, true);
        CHECK(per == 0 || (per < nb && slice_width(per, n + 12345, true) == 0));
    }
    CHECK(initial_kprime(10, kRows, 64) == 32 && initial_kprime(1, kRows, 64) == 32 && initial_kprime(10, 7, 64) == 7 && initial_kprime(10, 0, 64) == 1);
    CHECK(initial_kprime(42, kRows, 64) == 64 && initial_kprime(56, kRows, 64) == 64 && initial_kprime(57, kRows, 64) == 79);
    CHECK(initial_kprime(56, 70, 64) == 64 && initial_kprime(56, 60, 64) == 60);
}

void stats_added()
{
    // every field a distinct prime
    const int64_t primes[32] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131};
    constexpr size_t kFields = sizeof(orr_search_stats) / sizeof(int64_t);
    static_assert(sizeof(orr_search_stats) == 128 && kFields == 16, "a new counter: decide how add_search_stats treats it");
    orr_search_stats into, lane;
    int64_t *a = reinterpret_cast<int64_t *>(&into), *b = reinterpret_cast<int64_t *>(&lane);
    for (size_t i = 0; i < kFields; ++i) { a[i] = primes[i]; b[i] = primes[kFields + i]; }
    const orr_search_stats first = into;
    add_search_stats(into, lane);
    add_search_stats(into, lane);
    CHECK(into.searches == first.searches + 2 * lane.searches && into.queries == first.queries + 2 * lane.queries);
    CHECK(into.passes == first.passes + 2 * lane.passes && into.requeried == first.requeried + 2 * lane.requeried);
    CHECK(into.overflowed_queries == first.overflowed_queries + 2 * lane.overflowed_queries);
    CHECK(into.buffer_growths == first.buffer_growths + 2 * lane.buffer_growths);
    CHECK(into.exact_pass_queries == first.exact_pass_queries + 2 * lane.exact_pass_queries);
    CHECK(into.survivors_total == first.survivors_total + 2 * lane.survivors_total);
    CHECK(into.survivor_samples == first.survivor_samples + 2 * lane.survivor_samples);
    CHECK(into.kw_hits_total == first.kw_hits_total + 2 * lane.kw_hits_total && into.kw_passes == first.kw_passes + 2 * lane.kw_passes);
    CHECK(into.survivors_max == lane.survivors_max && into.survivor_capacity == lane.survivor_capacity);    // (the lane's primes are the larger)
    CHECK(into.pass_mode == first.pass_mode && into.vocab_tokens == first.vocab_tokens && into.reserved[0] == first.reserved[0]);
    // 11 sums and 2 maxima changed, 3 fields stayed: all 16
    size_t changed = 0;
    for (size_t i = 0; i < kFields; ++i) changed += a[i] != reinterpret_cast<const int64_t *>(&first)[i];
    CHECK(changed == 13);
    orr_search_stats fresh{};
    add_search_stats(fresh, lane);
    CHECK(fresh.pass_mode == lane.pass_mode);                         // the first lane that has one
}

const struct { const char *name; void (*run)(); } kScenarios[] = {
    {"rungs_in_order", rungs_in_order},
    {"mixed_causes", mixed_causes},
    {"growth_refused", growth_refused},
    {"three_shards", three_shards},
    {"repeat_only_if_grown", repeat_only_if_grown},
    {"termination", termination},
    {"old_against_new", old_against_new},
    {"survivors_accounted", survivors_accounted},
    {"slices_and_first_kprime", slices_and_first_kprime},
    {"stats_added", stats_added},
};

}  // namespace

int main(int argc, char **argv)
{
    for (const auto &s : kScenarios) {
        if (argc != 2 || strcmp(argv[1], s.name) != 0) continue;
        s.run();
        printf("%s ok\n", s.name);
        return 0;
    }
    fprintf(stderr, "usage: orr_escalation_selftest <scenario>, one of:\n");
    for (const auto &s : kScenarios) fprintf(stderr, "  %s\n", s.name);
    return 2;
}
