// orr_per_key_plan_selftest -- the rules of a per-key search (orr_per_key_plan.h) on the CPU, against brute force: the argument
// order, the union table with its slot masks and its lookup, the word / ballot rule of keys_exclude, and the rounds' result
// equal to the one-walk definition for random key assignments, caps and pools.  No HIP, no GPU; tests/test_per_key_cpu.py runs it.
#include "../orr_per_key_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace per_key;

static long g_fail = 0;
#define CHECK(c)                                                                                                                  \
    do {                                                                                                                          \
        if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); }                                      \
    } while (0)

static void test_arguments()
{
    CHECK(first_invalid(true, 99, 0, 0, true) == 1);
    CHECK(first_invalid(false, 99, 0, 0, true) == 2);
    CHECK(first_invalid(false, 99, 57, 0, true) == 2);
    CHECK(first_invalid(false, 99, -1, 0, true) == 2);
    CHECK(first_invalid(false, 57, 56, 0, true) == 3);
    CHECK(first_invalid(false, 2, 1, 0, true) == 3);
    CHECK(first_invalid(false, 10, 10, 0, true) == 4);
    CHECK(first_invalid(false, 10, 10, -5, true) == 4);
    CHECK(first_invalid(false, 10, 10, 1, true) == 5);
    CHECK(first_invalid(false, 10, 10, 1, false) == 0);
    CHECK(first_invalid(false, 0, 1, INT32_MAX, false) == 0);
    CHECK(first_invalid(false, -3, 1, 1, false) == 0);
    CHECK(first_invalid(false, 56, 56, 56, false) == 0);
    CHECK(first_invalid_scope_keys(true, -1, true, true) == 1);
    CHECK(first_invalid_scope_keys(false, -1, true, true) == 2);
    CHECK(first_invalid_scope_keys(false, kMaxScopeKeys + 1, true, true) == 2);
    CHECK(first_invalid_scope_keys(false, 3, true, true) == 3);
    CHECK(first_invalid_scope_keys(false, 3, false, true) == 4);
    CHECK(first_invalid_scope_keys(false, 0, true, true) == 4);
    CHECK(first_invalid_scope_keys(false, 0, true, false) == 0);
    CHECK(first_invalid_scope_keys(false, kMaxScopeKeys, false, false) == 0);
    CHECK(take_of(0) == 1 && take_of(-4) == 1 && take_of(1) == 1 && take_of(10) == 10);
    CHECK(kMaxPool == 56 && kBlockRows == kBlockThreads * 8 && kBlockWords % 4 == 0);
    CHECK(table_in_lds(0) && table_in_lds(kLdsTable) && !table_in_lds(kLdsTable + 1));
}

// the union table and its lookup against a brute-force search of every slot's set
static long test_table(std::mt19937_64 &rng)
{
    long lookups = 0;
    const int64_t special[] = {0, -1, INT64_MAX, INT64_MIN + 1, kNone};
    for (int rep = 0; rep < 300; ++rep) {
        const int S = 1 + (int)(rng() % kMaxSlots);
        const int span = 1 + (int)(rng() % 200);
        std::vector<std::set<int64_t>> closed((size_t)S);
        for (int s = 0; s < S; ++s) {
            const int n = (int)(rng() % 40);
            for (int i = 0; i < n; ++i) {
                const uint64_t r = rng();
                closed[(size_t)s].insert(r % 7 == 0 ? special[(r >> 8) % 5] : (int64_t)((r >> 8) % (uint64_t)span) - span / 2);
            }
        }
        if (rep % 10 == 0)                              // a key closed by every slot
            for (int s = 0; s < S; ++s) closed[(size_t)s].insert(12345);
        std::vector<const std::set<int64_t> *> ptr;
        for (auto &c : closed) ptr.push_back(&c);
        std::vector<int64_t> keys;
        std::vector<uint64_t> masks;
        build_table(ptr, keys, masks);
        CHECK(keys.size() == masks.size());
        for (size_t i = 0; i < keys.size(); ++i) {
            CHECK(keys[i] != kNone && masks[i] != 0ull);
            if (i) CHECK(keys[i - 1] < keys[i]);
        }
        std::vector<int64_t> probes(special, special + 5);
        for (int i = 0; i < 300; ++i) probes.push_back((int64_t)(rng() % (uint64_t)(span + 20)) - span / 2 - 10);
        probes.push_back(12345);
        for (int64_t k : probes) {
            uint64_t want = 0;
            if (k != kNone)
                for (int s = 0; s < S; ++s) want |= (uint64_t)closed[(size_t)s].count(k) << s;
            const uint64_t got = table_mask(keys.data(), masks.data(), (int32_t)keys.size(), k);
            CHECK(got == want);
            for (int s = 0; s < S; ++s) CHECK(slot_closed(got, s) == (((want >> s) & 1ull) != 0ull));
            ++lookups;
        }
        CHECK(table_mask(nullptr, nullptr, 0, 5) == 0ull);
    }
    // the member table: sorted, distinct, kNone a key like any other
    const int64_t list[] = {5, kNone, 5, -1, INT64_MAX, -1, 0};
    const std::vector<int64_t> t = member_table(list, 7);
    CHECK(t.size() == 5 && t[0] == kNone && t[1] == -1 && t[2] == 0 && t[3] == 5 && t[4] == INT64_MAX);
    CHECK(table_find(t.data(), 5, kNone) == 0 && table_find(t.data(), 5, 5) == 3 && table_find(t.data(), 5, 4) == -1);
    CHECK(table_find(t.data(), 0, 4) == -1);
    CHECK(member_table(list, 0).empty());
    return lookups;
}

// keys_exclude's words as the kernel forms them (a mask per row, one ballot per slot and wave, exclude_bits) against
// "base AND NOT the rows whose key slot s has closed", bit by bit
static long test_exclude_words(std::mt19937_64 &rng)
{
    long words = 0;
    for (int rep = 0; rep < 200; ++rep) {
        const int S = 1 + (int)(rng() % kMaxSlots);
        const int n_rows = 1 + (int)(rng() % 700);
        const int n_words = ((n_rows + 31) / 32 + 3) / 4 * 4;
        std::vector<int64_t> key((size_t)n_rows);
        for (auto &k : key) k = (rng() % 20 == 0) ? kNone : (int64_t)(rng() % 30);
        std::vector<std::set<int64_t>> closed((size_t)S);
        for (int s = 0; s < S; ++s)
            for (int i = (int)(rng() % 6); i > 0; --i) closed[(size_t)s].insert((int64_t)(rng() % 30));
        std::vector<const std::set<int64_t> *> ptr;
        for (auto &c : closed) ptr.push_back(&c);
        std::vector<int64_t> tk;
        std::vector<uint64_t> tm;
        build_table(ptr, tk, tm);
        std::vector<uint32_t> base((size_t)n_words, 0u);
        for (int r = 0; r < n_rows; ++r)
            if (rng() % 4) base[(size_t)(r >> 5)] |= 1u << (r & 31);
        for (int w0 = 0; w0 < n_words; w0 += 2) {      // a wave: 64 rows, two words
            uint64_t m[64];
            uint64_t any = 0;
            for (int l = 0; l < 64; ++l) {
                const int r = w0 * 32 + l;
                m[l] = table_mask(tk.data(), tm.data(), (int32_t)tk.size(), r < n_rows ? key[(size_t)r] : kNone);
                any |= m[l];
            }
            const uint64_t b = (uint64_t)base[(size_t)w0] | ((uint64_t)base[(size_t)w0 + 1] << 32);
            for (int s = 0; s < S; ++s) {
                uint64_t got = b;                       // a slot outside the wave's OR copies the base
                if ((any >> s) & 1ull) {
                    uint64_t ballot = 0;
                    for (int l = 0; l < 64; ++l) ballot |= (uint64_t)slot_closed(m[l], s) << l;
                    got = exclude_bits(b, ballot);
                }
                uint64_t want = 0;
                for (int l = 0; l < 64; ++l) {
                    const int r = w0 * 32 + l;
                    if (r >= n_rows || !((b >> l) & 1ull)) continue;
                    if (key[(size_t)r] != kNone && closed[(size_t)s].count(key[(size_t)r])) continue;
                    want |= 1ull << l;
                }
                CHECK(got == want);
                ++words;
            }
        }
    }
    return words;
}

// The rounds against the one-walk definition.  A ranking of n rows with keys in runs; round r > 1 sees the first `pool` rows of
// the ranking without closed keys and seen positions (what keys_exclude and keys_clear_seen leave of the frozen set).
static void test_rounds(std::mt19937_64 &rng, long &cases, long &multi, long &max_rounds, long &short_counts)
{
    for (int rep = 0; rep < 6000; ++rep) {
        const int n = (int)(rng() % 400);
        const int pool = 1 + (int)(rng() % kMaxPool);
        const int take = 1 + (int)(rng() % pool);
        const int cap = (rng() % 3 == 0) ? 1 + (int)(rng() % 56) : 1 + (int)(rng() % 3);
        const int max_run = 1 + (int)(rng() % 70);
        std::vector<int64_t> key((size_t)n);
        const int64_t special[] = {0, -1, INT64_MAX, INT64_MIN + 1};
        int64_t next = 100;
        for (int i = 0; i < n;) {
            const int run = 1 + (int)(rng() % max_run);
            const uint64_t r = rng();
            const int64_t k = r % 20 == 0 ? kNone : (r % 9 == 0 ? special[(r >> 8) % 4] : (r % 5 == 0 && next > 100 ? 100 + (int64_t)((r >> 8) % (uint64_t)(next - 100)) : next++));
            for (int j = 0; j < run && i < n; ++j, ++i) key[(size_t)i] = k;
        }
        const std::vector<int32_t> want = walk_all(n, key.data(), take, cap);
        {                                               // the definition itself against a direct count
            std::map<int64_t, int> c;
            for (int32_t r : want) if (key[(size_t)r] != kNone) CHECK(++c[key[(size_t)r]] <= cap);
            CHECK((int)want.size() <= take);
            if ((int)want.size() < take) {              // the candidates ran out: every row left out is over its cap
                std::set<int32_t> in(want.begin(), want.end());
                for (int r = 0; r < n; ++r) if (!in.count(r)) CHECK(key[(size_t)r] != kNone && c[key[(size_t)r]] == cap);
                ++short_counts;
            }
        }
        State st;
        while (!st.finished) {
            std::set<int64_t> seen(st.seen.begin(), st.seen.end());
            std::vector<int64_t> rk, rp;
            std::vector<int32_t> num;
            for (int r = 0; r < n && (int)rk.size() < pool; ++r) {
                if (seen.count(r)) continue;
                if (key[(size_t)r] != kNone && st.closed.count(key[(size_t)r])) continue;
                rk.push_back(key[(size_t)r]); rp.push_back(r); num.push_back(r);
            }
            const size_t had = st.kept.size();
            walk_round(st, (int32_t)rk.size(), rk.data(), rp.data(), num.data(), take, cap, pool);
            CHECK(st.finished || st.kept.size() > had);     // every round keeps at least one row
            if (st.rounds > take) { CHECK(false); break; }
        }
        CHECK(st.kept == want);
        CHECK(st.rounds >= 1 && st.rounds <= take);
        if (cap >= take) CHECK(st.rounds == 1 && (int)want.size() == std::min(n, take));
        ++cases;
        if (st.rounds > 1) ++multi;
        if (st.rounds > max_rounds) max_rounds = st.rounds;
    }
    // the planted shape: five documents of 70 rows on top, max_per_key 1, topk 10, pool 16: six rounds
    std::vector<int64_t> key;
    for (int d = 0; d < 5; ++d) for (int i = 0; i < 70; ++i) key.push_back(1000 + d);
    for (int i = 0; i < 200; ++i) key.push_back(2000 + i);
    State st;
    while (!st.finished) {
        std::set<int64_t> seen(st.seen.begin(), st.seen.end());
        std::vector<int64_t> rk, rp;
        std::vector<int32_t> num;
        for (int r = 0; r < (int)key.size() && (int)rk.size() < 16; ++r) {
            if (seen.count(r) || st.closed.count(key[(size_t)r])) continue;
            rk.push_back(key[(size_t)r]); rp.push_back(r); num.push_back(r);
        }
        walk_round(st, (int32_t)rk.size(), rk.data(), rp.data(), num.data(), 10, 1, 16);
    }
    CHECK(st.rounds == 6 && st.kept.size() == 10 && st.kept[4] == 280 && st.kept[5] == 350 && st.kept[9] == 354);
}

int main()
{
    std::mt19937_64 rng(20240611);
    test_arguments();
    const long lookups = test_table(rng);
    const long words = test_exclude_words(rng);
    long cases = 0, multi = 0, max_rounds = 0, short_counts = 0;
    test_rounds(rng, cases, multi, max_rounds, short_counts);
    printf("table lookups checked: %ld\n", lookups);
    printf("exclusion words checked: %ld\n", words);
    printf("round cases checked: %ld (more than one round: %ld, most rounds: %ld, candidates ran out: %ld)\n", cases, multi, max_rounds,
           short_counts);
    if (g_fail) { printf("orr_per_key_plan_selftest: %ld FAILED\n", g_fail); return 1; }
    printf("orr_per_key_plan_selftest: ok\n");
    return 0;
}
