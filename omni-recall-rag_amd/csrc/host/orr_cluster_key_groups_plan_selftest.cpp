// orr_cluster_key_groups_plan_selftest -- what a cluster adds to the key groups (orr_cluster_key_groups_plan.h) on the CPU: the
// argument order, the merge of the shards' group lists, the cut of a key at a shard border against a member-by-member count, the
// records of a shard executed on the host (run_records) against key_groups::sum_blocked over the concatenated members, bit for
// bit, and a crafted input on which the chained sum differs from "blocks restart at the border" and from "per-shard sums added
// up".  No HIP, no GPU; tests/test_cluster_key_groups_cpu.py runs it.
#include "../orr_cluster_key_groups_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace cluster_key_groups;
using key_groups::Block;
using key_groups::Fold;
using key_groups::kDirect;

static long g_fail = 0;
#define CHECK(c)                                                                                                                  \
    do {                                                                                                                          \
        if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); }                                      \
    } while (0)

static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

static void test_arguments()
{
    for (int64_t cap : {(int64_t)-1, (int64_t)0, (int64_t)5})
        for (int m = 0; m < 32; ++m)
            CHECK(first_invalid_groups(cap, m & 1, m & 2, m & 4, m & 8, m & 16) == key_groups::first_invalid_groups(cap, m & 1, m & 2, m & 4, m & 8, m & 16));
    for (int32_t n : {-1, 0, 3, key_groups::kMaxKeys, key_groups::kMaxKeys + 1})
        for (int m = 0; m < 8; ++m)
            CHECK(first_invalid_centroids(n, m & 1, m & 2, m & 4) == key_groups::first_invalid_centroids(n, m & 1, m & 2, m & 4));
    for (int m = 0; m < 4; ++m) CHECK(first_invalid_scope_centroid(m & 1, m & 2) == key_groups::first_invalid_scope_centroid(m & 1, m & 2));
    CHECK(first_invalid_groups(-1, true, true, true, true, true) == 1 && first_invalid_groups(0, true, true, false, false, true) == 4);
    CHECK(first_invalid_centroids(3, true, true, true) == 2 && first_invalid_centroids(0, true, true, true) == 4);
    CHECK(first_invalid_scope_centroid(true, true) == 1 && first_invalid_scope_centroid(false, true) == 2);
}

static void test_merge_groups()
{
    // a key on all shards (7), on one shard (3, 9), an empty shard, the extreme keys
    const std::vector<std::vector<int64_t>> keys = {{INT64_MIN + 1, 3, 7}, {}, {7, 9}, {7, INT64_MAX}};
    const std::vector<std::vector<int64_t>> rows = {{2, 5, 1}, {}, {10, 4}, {100, 6}};
    std::vector<int64_t> k, r;
    CHECK(merge_groups(keys, rows, 100, k, r) == 5);
    CHECK((k == std::vector<int64_t>{INT64_MIN + 1, 3, 7, 9, INT64_MAX}) && (r == std::vector<int64_t>{2, 5, 111, 4, 6}));
    CHECK(merge_groups(keys, rows, 0, k, r) == 5 && k.empty() && r.empty());
    CHECK(merge_groups(keys, rows, 3, k, r) == 5);
    CHECK((k == std::vector<int64_t>{INT64_MIN + 1, 3, 7}) && (r == std::vector<int64_t>{2, 5, 111}));
    CHECK(merge_groups(keys, rows, 5, k, r) == 5 && k.size() == 5);
    CHECK(merge_groups({}, {}, 4, k, r) == 0 && k.empty());
    CHECK(merge_groups({{}, {}}, {{}, {}}, 4, k, r) == 0 && k.empty());
    CHECK(merge_groups({{-1, 0}}, {{1, 2}}, 4, k, r) == 2 && (k == std::vector<int64_t>{-1, 0}) && (r == std::vector<int64_t>{1, 2}));
}

// the cut, counted member by member: member i of the key (0 .. total) lies in block i / 256
static long test_cut()
{
    long checked = 0;
    const int64_t befores[] = {0, 1, 255, 256, 257, 511, 512}, counts[] = {0, 1, 2, 255, 256, 257, 600};
    for (int64_t before : befores)
        for (int64_t count : counts)
            for (int64_t after : {(int64_t)0, (int64_t)1, (int64_t)300}) {
                const int64_t total = before + count + after, end = before + count;
                const Cut c = cut(before, count, total);
                ++checked;
                if (count == 0) {
                    CHECK(c.head == 0 && c.n_free == 0 && c.n_close == 0 && !c.head_closes && c.open == kOpenNone && !c.seed_s && !c.seed_p);
                    continue;
                }
                int64_t head = 0, free_blocks = 0, closing = 0;
                bool head_closes = false;
                uint32_t open = kOpenNone;
                const int64_t first_block = before / kBlock, last_block = (end - 1) / kBlock;
                for (int64_t b = first_block; b <= last_block; ++b) {
                    const int64_t lo = b * kBlock > before ? b * kBlock : before, hi = (b + 1) * kBlock < end ? (b + 1) * kBlock : end;
                    const bool is_head = b * kBlock < before;       // it began on a shard in front
                    const bool closes = hi == (b + 1) * kBlock || hi == total;
                    if (is_head) { head = hi - lo; head_closes = closes; if (!closes) open = kOpenHead; }
                    else { ++free_blocks; if (closes) ++closing; else open = kOpenFree; }
                }
                CHECK(c.head == head && c.n_free == free_blocks && c.n_close == closing && c.head_closes == head_closes && c.open == open);
                CHECK(c.seed_s == (before > 0) && c.seed_p == (head > 0));
                CHECK(c.head >= 0 && c.head < kBlock);
            }
    const Cut edge = cut(256, 3, 1000);                 // a border on a block edge: S seeded, no head, a free block left open
    CHECK(edge.head == 0 && edge.seed_s && !edge.seed_p && edge.n_free == 1 && edge.n_close == 0 && edge.open == kOpenFree);
    const Cut stays = cut(259, 10, 1000);               // too few members to close the open block
    CHECK(stays.head == 10 && !stays.head_closes && stays.open == kOpenHead && stays.n_free == 0 && stays.seed_p);
    const Cut tail = cut(269, 731, 1000);               // a head that closes, then free blocks, then the key's tail
    CHECK(tail.head == 243 && tail.head_closes && tail.n_free == 2 && tail.n_close == 2 && tail.open == kOpenNone);
    return checked;
}

// key 0: `members` cut into parts; key 1 (slot 1): `other`, wholly on shard `other_on`.  Every shard's records run on the host.
struct Chained {
    std::vector<double> s0, s1;
    long chain_records = 0;
};
static Chained run_chain(const std::vector<float> &emb, int32_t dim, const std::vector<int64_t> &members, const std::vector<int64_t> &parts,
                         const std::vector<int64_t> &other, int32_t other_on)
{
    Chained out;
    const int64_t total[2] = {(int64_t)members.size(), (int64_t)other.size()};
    std::vector<double> state((size_t)2 * dim, 7.0), answer0((size_t)dim, 0.0), answer1((size_t)dim, 0.0);
    const int32_t slot_state[2] = {0, -1};
    int64_t before0 = 0;
    bool spanning = false;
    for (int64_t p : parts) spanning = spanning || spans(p, total[0]);
    for (size_t g = 0; g < parts.size(); ++g) {
        std::vector<uint32_t> pos;
        for (int64_t i = 0; i < parts[g]; ++i) pos.push_back((uint32_t)members[(size_t)(before0 + i)]);
        const bool has_other = (int32_t)g == other_on;
        if (has_other) for (int64_t m : other) pos.push_back((uint32_t)m);
        const int64_t count[2] = {parts[g], has_other ? total[1] : 0}, first[2] = {0, parts[g]}, before[2] = {before0, 0};
        Records r;
        records_of(2, count, first, before, total, slot_state, nullptr, r);
        for (const Block &b : r.blocks) {
            CHECK(b.len >= 1 && b.len <= (uint32_t)kBlock && (size_t)b.first + b.len <= pos.size());
            CHECK(b.part == kDirect || b.part < r.n_parts);
            if (b.slot == 0 && spanning) CHECK(b.part != kDirect);
        }
        for (const Chain &c : r.chains) {
            CHECK(c.state == 0 && c.head_len < (uint32_t)kBlock && (size_t)c.head_first + c.head_len <= pos.size());
            CHECK((size_t)c.part0 + c.n_close + (chain_open(c.flags) == kOpenFree ? 1 : 0) <= r.n_parts);
        }
        if (!spans(parts[g], total[0])) CHECK(r.chains.empty());
        else CHECK(r.chains.size() == 1);
        if (parts[g] == total[0] && parts[g] > 0) {     // wholly here: exactly blocks_of's records
            std::vector<Block> wb; std::vector<Fold> wf; uint32_t np = 0;
            key_groups::blocks_of(total[0], 0, 0u, wb, wf, np);
            size_t same = 0;
            for (size_t i = 0; i < wb.size() && i < r.blocks.size(); ++i)
                same += r.blocks[i].first == wb[i].first && r.blocks[i].len == wb[i].len && r.blocks[i].slot == wb[i].slot &&
                        r.blocks[i].index == wb[i].index && r.blocks[i].part == wb[i].part;
            CHECK(same == wb.size());
        }
        out.chain_records += (long)r.chains.size();
        std::vector<double> sums((size_t)2 * dim, 0.0), prt((size_t)(r.n_parts + 1) * dim, -3.0);
        run_records(r, emb.data(), dim, pos.data(), sums.data(), prt.data(), state.data());
        if (parts[g] == total[0]) answer0.assign(sums.begin(), sums.begin() + dim);
        if (has_other) answer1.assign(sums.begin() + dim, sums.end());
        before0 += parts[g];
    }
    if (spanning) answer0.assign(state.begin(), state.begin() + dim);
    out.s0 = answer0; out.s1 = answer1;
    return out;
}

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) if (bits_of(a[i]) != bits_of(b[i])) return false;
    return true;
}

// "blocks restart at the border" (restart) and "per-shard blocked sums added up" (!restart)
static std::vector<double> wrong_order(const std::vector<float> &emb, int32_t dim, const std::vector<int64_t> &members, const std::vector<int64_t> &parts, bool restart)
{
    std::vector<double> S((size_t)dim, 0.0), one((size_t)dim);
    int64_t at = 0;
    for (int64_t p : parts) {
        if (restart) {
            for (int64_t b0 = 0; b0 < p; b0 += kBlock) {
                const int64_t len = p - b0 < kBlock ? p - b0 : kBlock;
                key_groups::sum_blocked(emb.data(), dim, members.data() + at + b0, len, one.data());
                for (int32_t d = 0; d < dim; ++d) { volatile double s = S[(size_t)d]; s = s + one[(size_t)d]; S[(size_t)d] = s; }
            }
        } else if (p > 0) {
            key_groups::sum_blocked(emb.data(), dim, members.data() + at, p, one.data());
            for (int32_t d = 0; d < dim; ++d) { volatile double s = S[(size_t)d]; s = s + one[(size_t)d]; S[(size_t)d] = s; }
        }
        at += p;
    }
    return S;
}

static void test_chain(long &cases, long &chains, long &told_apart)
{
    const int32_t dim = 5, rows = 1400;
    std::vector<float> emb((size_t)rows * dim);
    for (float &v : emb) v = (float)((uni() - 0.5) * std::pow(10.0, uni() * 30.0 - 15.0));
    emb[3 * dim + 1] = INFINITY;
    emb[9 * dim + 2] = -0.0f;
    const int64_t ns[] = {1, 255, 256, 257, 513, 1000};
    for (int64_t n : ns)
        for (int n_parts = 1; n_parts <= 5; ++n_parts)
            for (int rep = 0; rep < 12; ++rep) {
                std::vector<int64_t> perm((size_t)rows);
                for (int32_t i = 0; i < rows; ++i) perm[(size_t)i] = i;
                for (int32_t i = rows - 1; i > 0; --i) std::swap(perm[(size_t)i], perm[(size_t)(rnd() % (uint64_t)(i + 1))]);
                const std::vector<int64_t> members(perm.begin(), perm.begin() + n);
                const int64_t n_other = (int64_t)(rnd() % 3 == 0 ? 0 : 1 + rnd() % 390);
                const std::vector<int64_t> other(perm.begin() + 1000, perm.begin() + 1000 + n_other);
                // cuts: random, with repeats (empty parts) and, every third time, on block edges or right behind them
                std::vector<int64_t> cuts;
                for (int i = 0; i + 1 < n_parts; ++i) {
                    int64_t c = (int64_t)(rnd() % (uint64_t)(n + 1));
                    if (rep % 3 == 1) c = (c / kBlock) * kBlock;
                    if (rep % 3 == 2 && i > 0) c = cuts.back() + (int64_t)(rnd() % 4);
                    cuts.push_back(c > n ? n : c);
                }
                for (size_t i = 0; i < cuts.size(); ++i) for (size_t j = i + 1; j < cuts.size(); ++j) if (cuts[j] < cuts[i]) std::swap(cuts[i], cuts[j]);
                std::vector<int64_t> parts;
                int64_t at = 0;
                for (int64_t c : cuts) { parts.push_back(c - at); at = c; }
                parts.push_back(n - at);
                const Chained got = run_chain(emb, dim, members, parts, other, (int32_t)(rnd() % (uint64_t)n_parts));
                std::vector<double> want0((size_t)dim), want1((size_t)dim);
                key_groups::sum_blocked(emb.data(), dim, members.data(), n, want0.data());
                key_groups::sum_blocked(emb.data(), dim, other.data(), n_other, want1.data());
                CHECK(same_bits(got.s0, want0));
                CHECK(same_bits(got.s1, want1));
                ++cases;
                chains += got.chain_records;
                bool on_edges = true;
                for (int64_t c : cuts) on_edges = on_edges && c % kBlock == 0;
                const bool a = !same_bits(wrong_order(emb, dim, members, parts, true), want0), b = !same_bits(wrong_order(emb, dim, members, parts, false), want0);
                if (on_edges) CHECK(!a);                // every cut on a block edge: the restarted blocks ARE the blocks
                told_apart += a && b;
            }
}

// 2^53, then ones: inside a block that began with 2^53 every + 1.0 is lost (a tie, to even), in a block from +0.0 the ones add up
static void test_crafted()
{
    const int32_t dim = 1;
    std::vector<float> emb(300, 1.0f);
    emb[0] = 9007199254740992.0f;
    std::vector<int64_t> members(300);
    for (int64_t i = 0; i < 300; ++i) members[(size_t)i] = i;
    const std::vector<int64_t> parts = {100, 200};
    const Chained got = run_chain(emb, dim, members, parts, {}, 0);
    double want = 0.0;
    key_groups::sum_blocked(emb.data(), dim, members.data(), 300, &want);
    CHECK(want == 9007199254740992.0 + 44.0);           // block 0: 2^53 + 255 lost ones; block 1: 44 ones
    CHECK(got.s0.size() == 1 && bits_of(got.s0[0]) == bits_of(want));
    const double restart = wrong_order(emb, dim, members, parts, true)[0], added = wrong_order(emb, dim, members, parts, false)[0];
    CHECK(restart == 9007199254740992.0 + 200.0 && added == 9007199254740992.0 + 200.0);
    CHECK(bits_of(restart) != bits_of(want) && bits_of(added) != bits_of(want));
}

int main()
{
    test_arguments();
    test_merge_groups();
    const long cuts = test_cut();
    long cases = 0, chains = 0, told_apart = 0;
    test_chain(cases, chains, told_apart);
    test_crafted();
    CHECK(told_apart > 0);
    printf("cuts checked: %ld\n", cuts);
    printf("chained cases checked: %ld (chain records run: %ld, told apart from both wrong orders: %ld)\n", cases, chains, told_apart);
    if (g_fail) { fprintf(stderr, "orr_cluster_key_groups_plan_selftest: %ld check(s) failed\n", g_fail); return 1; }
    printf("orr_cluster_key_groups_plan_selftest: ok\n");
    return 0;
}
