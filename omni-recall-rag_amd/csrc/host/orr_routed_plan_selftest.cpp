// orr_routed_plan_selftest -- the rules of a routed search (orr_routed_plan.h) on the CPU: the argument order, the canonical
// set of a route, the slots by first appearance, the slices of at most 64 slots, the union table, include_bits against a
// bit-by-bit emulation of one keys_include workgroup.  No HIP, no GPU; tests/test_routed_cpu.py runs it.
//
// With arguments `slots IN OUT` it is a driver for that test's own restatement: IN holds int64 B, route, route_keys[B][route],
// route_n[B]; OUT receives int64 n_slots, slot_of[B], per slot its size and keys, n_slices, and per slice slot0, n_slots, nq,
// queries[nq], query_slot[nq], n_tab, tab_keys[n_tab], tab_masks[n_tab].  With `include IN OUT`: IN holds int64 n, base[n],
// in[n] (64-bit words); OUT receives include_bits of each pair.
#include "../orr_routed_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace routed;

static long g_fail = 0;
#define CHECK(c)                                                                                                                  \
    do {                                                                                                                          \
        if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); }                                      \
    } while (0)

static void test_arguments()
{
    CHECK(first_invalid(true, 0, true, true) == 1);
    CHECK(first_invalid(false, 0, true, true) == 2);
    CHECK(first_invalid(false, kMaxRoute + 1, false, false) == 2);
    CHECK(first_invalid(false, -5, false, false) == 2);
    CHECK(first_invalid(false, 1, true, true) == 3);
    CHECK(first_invalid(false, kMaxRoute, false, true) == 4);
    CHECK(first_invalid(false, 1, false, false) == 0 && first_invalid(false, kMaxRoute, false, false) == 0);
    CHECK(kMaxRoute == 1024 && kNone == INT64_MIN);
    CHECK(include_bits(0xF0F0ull, 0xFF00ull) == 0xF000ull);
    CHECK(include_bits(~0ull, 0x8000000000000001ull) == 0x8000000000000001ull && include_bits(0ull, ~0ull) == 0ull);
}

static void test_canonical_and_slots()
{
    const int64_t d[] = {7, kNone, 3, 7, INT64_MAX, kNone + 1, 3};
    const std::set<int64_t> c = canonical(d, 7);
    const std::set<int64_t> want = {kNone + 1, 3, 7, INT64_MAX};
    CHECK(c == want);
    CHECK(canonical(d, 0).empty());
    CHECK(canonical(d + 1, 1).empty());                 // kNone alone: the empty set
    // route 3, six queries: {5, 9}, {9, 5, 5}, {} (n 0), {kNone}, {1}, {9, 5, kNone}
    const int64_t rk[] = {5, 9, kNone,   9, 5, 5,   4, 4, 4,   kNone, 8, 8,   1, kNone, kNone,   9, 5, kNone};
    const int32_t rn[] = {2, 3, 0, 1, 1, 3};
    const Slots s = slots(6, 3, rk, rn);
    CHECK(s.sets.size() == 2);
    const int32_t want_slot[] = {0, 0, kNoSlot, kNoSlot, 1, 0};
    for (int b = 0; b < 6; ++b) CHECK(s.slot_of[(size_t)b] == want_slot[b]);
    CHECK((s.sets[0] == std::set<int64_t>{5, 9}) && (s.sets[1] == std::set<int64_t>{1}));
    const std::vector<Slice> sl = slices(s);
    CHECK(sl.size() == 1 && sl[0].slot0 == 0 && sl[0].n_slots == 2);
    CHECK((sl[0].queries == std::vector<int32_t>{0, 1, 4, 5}) && (sl[0].query_slot == std::vector<int32_t>{0, 0, 1, 0}));
    std::vector<int64_t> tk;
    std::vector<uint64_t> tm;
    slice_table(s, sl[0], tk, tm);
    CHECK((tk == std::vector<int64_t>{1, 5, 9}) && (tm == std::vector<uint64_t>{2, 1, 1}));
    // an all-empty batch: no slot, no slice
    const int32_t zero[] = {0, 0, 0, 0, 0, 0};
    const Slots e = slots(6, 3, rk, zero);
    CHECK(e.sets.empty() && slices(e).empty());
    for (int b = 0; b < 6; ++b) CHECK(e.slot_of[(size_t)b] == kNoSlot);
}

static void test_slices()
{
    // 130 distinct sets, each named by two queries (b and b + 130), route 2: slices of 64, 64 and 2
    const int32_t B = 260;
    std::vector<int64_t> rk((size_t)B * 2);
    std::vector<int32_t> rn((size_t)B, 2);
    for (int32_t b = 0; b < B; ++b) {                   // {10 (b mod 130), 5}, in either order
        rk[(size_t)b * 2 + (b < 130 ? 0 : 1)] = (b % 130) * 10;
        rk[(size_t)b * 2 + (b < 130 ? 1 : 0)] = 5;
    }
    const Slots s = slots(B, 2, rk.data(), rn.data());
    CHECK(s.sets.size() == 130);
    for (int32_t b = 0; b < B; ++b) CHECK(s.slot_of[(size_t)b] == b % 130);
    const std::vector<Slice> sl = slices(s);
    CHECK(sl.size() == 3 && sl[0].n_slots == 64 && sl[1].n_slots == 64 && sl[2].n_slots == 2);
    CHECK(sl[0].slot0 == 0 && sl[1].slot0 == 64 && sl[2].slot0 == 128);
    size_t total = 0;
    for (const Slice &c : sl) {
        CHECK(c.queries.size() == (size_t)c.n_slots * 2 && c.query_slot.size() == c.queries.size());
        for (size_t i = 0; i < c.queries.size(); ++i) {
            CHECK(i == 0 || c.queries[i - 1] < c.queries[i]);
            CHECK(c.query_slot[i] >= 0 && c.query_slot[i] < c.n_slots && c.slot0 + c.query_slot[i] == s.slot_of[(size_t)c.queries[i]]);
        }
        std::vector<int64_t> tk;
        std::vector<uint64_t> tm;
        slice_table(s, c, tk, tm);
        CHECK(tk.size() == (size_t)c.n_slots + 1);
        // key 5 is routed by every slot of the slice
        const uint64_t all = c.n_slots == 64 ? ~0ull : (1ull << c.n_slots) - 1ull;
        const int32_t i5 = per_key::table_find(tk.data(), (int32_t)tk.size(), 5);
        CHECK(i5 >= 0 && tm[(size_t)i5] == all);
        total += c.queries.size();
    }
    CHECK(total == (size_t)B);
}

// One keys_include workgroup, bit by bit: per slot the words of rows whose key the slot routed to, ANDed with the base.
static void test_include_emulation()
{
    std::mt19937_64 rng(12345);
    const int32_t S = 5, rows = per_key::kBlockRows - 37;
    std::vector<std::set<int64_t>> sets((size_t)S);
    for (int32_t s = 0; s < S; ++s)
        for (int i = 0; i < 3; ++i) sets[(size_t)s].insert((int64_t)(rng() % 40));
    std::vector<const std::set<int64_t> *> ptr;
    for (auto &x : sets) ptr.push_back(&x);
    std::vector<int64_t> tk;
    std::vector<uint64_t> tm;
    per_key::build_table(ptr, tk, tm);
    std::vector<int64_t> key((size_t)rows);
    for (auto &k : key) { k = (int64_t)(rng() % 48); if (k >= 44) k = kNone; }
    std::vector<uint64_t> base(per_key::kBlockWords / 2);
    for (auto &w : base) w = rng();
    for (int32_t s = 0; s < S; ++s)
        for (int32_t w = 0; w < per_key::kBlockWords / 2; ++w) {
            uint64_t in = 0, want = 0;
            for (int l = 0; l < 64; ++l) {
                const int64_t r = (int64_t)w * 64 + l;
                const int64_t k = r < rows ? key[(size_t)r] : kNone;
                if (per_key::slot_closed(per_key::table_mask(tk.data(), tm.data(), (int32_t)tk.size(), k), s)) in |= 1ull << l;
                if (r < rows && k != kNone && sets[(size_t)s].count(k) && ((base[(size_t)w] >> l) & 1ull)) want |= 1ull << l;
            }
            CHECK(include_bits(base[(size_t)w], in) == want);
        }
}

static bool read_i64(FILE *f, std::vector<int64_t> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), 8, n, f) == n;
}

static int drive_slots(const char *in, const char *out)
{
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    int64_t head[2] = {0, 0};
    std::vector<int64_t> rk, rn64;
    bool ok = fread(head, 8, 2, f) == 2 && head[0] >= 0 && head[1] >= 1 && head[0] <= (1 << 20) && head[1] <= kMaxRoute;
    ok = ok && read_i64(f, rk, (size_t)(head[0] * head[1])) && read_i64(f, rn64, (size_t)head[0]);
    fclose(f);
    if (!ok) return 2;
    const int32_t B = (int32_t)head[0], route = (int32_t)head[1];
    std::vector<int32_t> rn(rn64.begin(), rn64.end());
    const Slots s = slots(B, route, rk.data(), rn.data());
    std::vector<int64_t> o;
    o.push_back((int64_t)s.sets.size());
    for (int32_t v : s.slot_of) o.push_back(v);
    for (const auto &set : s.sets) {
        o.push_back((int64_t)set.size());
        for (int64_t k : set) o.push_back(k);
    }
    const std::vector<Slice> sl = slices(s);
    o.push_back((int64_t)sl.size());
    for (const Slice &c : sl) {
        o.push_back(c.slot0); o.push_back(c.n_slots); o.push_back((int64_t)c.queries.size());
        for (int32_t q : c.queries) o.push_back(q);
        for (int32_t q : c.query_slot) o.push_back(q);
        std::vector<int64_t> tk;
        std::vector<uint64_t> tm;
        slice_table(s, c, tk, tm);
        o.push_back((int64_t)tk.size());
        for (int64_t k : tk) o.push_back(k);
        for (uint64_t m : tm) o.push_back((int64_t)m);
    }
    FILE *w = fopen(out, "wb");
    if (!w) return 2;
    ok = fwrite(o.data(), 8, o.size(), w) == o.size();
    ok = fclose(w) == 0 && ok;
    return ok ? 0 : 2;
}

static int drive_include(const char *in, const char *out)
{
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    int64_t n = 0;
    std::vector<int64_t> base, inc;
    bool ok = fread(&n, 8, 1, f) == 1 && n >= 0 && n <= (1 << 24) && read_i64(f, base, (size_t)n) && read_i64(f, inc, (size_t)n);
    fclose(f);
    if (!ok) return 2;
    std::vector<uint64_t> o((size_t)n);
    for (int64_t i = 0; i < n; ++i) o[(size_t)i] = include_bits((uint64_t)base[(size_t)i], (uint64_t)inc[(size_t)i]);
    FILE *w = fopen(out, "wb");
    if (!w) return 2;
    ok = n == 0 || fwrite(o.data(), 8, (size_t)n, w) == (size_t)n;
    ok = fclose(w) == 0 && ok;
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "slots") == 0) return drive_slots(argv[2], argv[3]);
    if (argc == 4 && strcmp(argv[1], "include") == 0) return drive_include(argv[2], argv[3]);
    test_arguments();
    test_canonical_and_slots();
    test_slices();
    test_include_emulation();
    if (g_fail) { fprintf(stderr, "orr_routed_plan_selftest: %ld failures\n", g_fail); return 1; }
    printf("orr_routed_plan_selftest: ok\n");
    return 0;
}
