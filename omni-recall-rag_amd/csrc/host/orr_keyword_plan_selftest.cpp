// orr_keyword_plan_selftest -- the host half of the keyword chain (orr_keyword_plan.h) on the CPU, against oracles written
// another way: the distinct terms against a std::map, the image against one built byte by byte, the lookup tables against a
// sort of tuples and a count per class, the choices and the hit list's rule at their edges.  No HIP, no GPU;
// tests/test_keyword_plan_cpu.py runs it.
//   --dump: reads "N" and N lines of hex (one term each, an empty line is the empty term) from stdin, prints the lookup tables
//   of those terms as fill_meta writes them (tests/test_vocab_lookup_theory.py compares them with its own restatement).
#include "../orr_keyword_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <random>
#include <string>
#include <tuple>

using namespace keyword;

static long g_fail = 0;
#define CHECK(c)                                                                                                                  \
    do {                                                                                                                          \
        if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); }                                      \
    } while (0)

// A batch as a caller hands it over: every term's bytes at a pool offset of its own (equal terms do NOT share bytes), `lead`
// terms of earlier queries in front of the batch's first.
struct Batch {
    std::vector<uint8_t> pool;
    std::vector<uint32_t> term_off, qoff;
    int32_t B = 0;
};
static Batch make_batch(const std::vector<std::string> &lead, const std::vector<std::vector<std::string>> &queries)
{
    Batch b;
    b.term_off.push_back(0);
    auto add = [&](const std::string &t) {
        b.pool.insert(b.pool.end(), t.begin(), t.end());
        b.term_off.push_back((uint32_t)b.pool.size());
    };
    for (auto &t : lead) add(t);
    b.qoff.push_back((uint32_t)lead.size());
    for (auto &q : queries) {
        for (auto &t : q) add(t);
        b.qoff.push_back((uint32_t)b.term_off.size() - 1);
    }
    b.B = (int32_t)queries.size();
    b.pool.push_back(0);                               // (never empty: data() is a pointer)
    return b;
}

// distinct_terms against a std::map: numbers in order of first appearance, the map per term, the offsets, the pool bytes
static void check_distinct(const std::vector<std::string> &lead, const std::vector<std::vector<std::string>> &queries)
{
    const Batch b = make_batch(lead, queries);
    Distinct d;
    CHECK(distinct_terms(b.pool.data(), b.term_off.data(), b.qoff.data(), b.B, d) == -1);
    std::map<std::string, uint32_t> number;
    std::vector<std::string> first;
    std::vector<uint32_t> want;
    size_t bytes = 0;
    for (auto &q : queries)
        for (auto &t : q) {
            auto it = number.find(t);
            if (it == number.end()) {
                it = number.emplace(t, (uint32_t)first.size()).first;
                first.push_back(t);
                bytes += t.size();
            }
            want.push_back(it->second);
        }
    CHECK(d.terms.size() == first.size());
    for (size_t i = 0; i < first.size() && i < d.terms.size(); ++i) CHECK(d.terms[i] == std::string_view(first[i]));
    CHECK(d.qmeta.size() == want.size() + queries.size() + 1);
    if (d.qmeta.size() != want.size() + queries.size() + 1) return;
    for (size_t i = 0; i < want.size(); ++i) CHECK(d.qmeta[i] == want[i]);
    uint32_t off = 0;
    for (size_t q = 0; q <= queries.size(); ++q) {
        CHECK(d.qmeta[want.size() + q] == off);
        if (q < queries.size()) off += (uint32_t)queries[q].size();
    }
    CHECK(d.pool_bytes == bytes);
}

static std::string random_term(std::mt19937_64 &rng)
{
    static const char *stems[] = {"a", "ab", "abc", "abcd", "abcde", "kubernetes", "kubernetesx", "net", "x", "\xc3\xa9", "\xff\x80", "0123456789abcdef",
                                  "0123456789abcdefg", "a-term-of-more-than-thirty-two-bytes-in-all"};
    std::string t = stems[rng() % 14];
    if (rng() % 3 == 0) t = t.substr(0, 1 + rng() % t.size());        // a prefix of another
    if (rng() % 2 == 0) t += std::to_string(rng() % 400);
    return t;
}

static void test_distinct(std::mt19937_64 &rng, long &lists, long &batches, long &repeats)
{
    // every list of 0 .. 6 terms over {"", "a", "ab"}: as one query, and split in two at every other position
    const std::string alpha[3] = {"", "a", "ab"};
    for (int len = 0; len <= 6; ++len) {
        int total = 1;
        for (int i = 0; i < len; ++i) total *= 3;
        for (int code = 0; code < total; ++code) {
            std::vector<std::string> list;
            for (int i = 0, c = code; i < len; ++i, c /= 3) list.push_back(alpha[c % 3]);
            check_distinct({}, {list});
            const size_t cut = (size_t)code % (list.size() + 1);
            check_distinct({"zz"}, {std::vector<std::string>(list.begin(), list.begin() + (long)cut), {}, std::vector<std::string>(list.begin() + (long)cut, list.end())});
            ++lists;
        }
    }
    // random batches of up to 3,000 terms: repeats within and across queries, prefixes, a query without terms, terms in front
    for (int rep = 0; rep < 60; ++rep) {
        const size_t n_terms = rep < 3 ? 3000 : rng() % 3001;
        const size_t B = 1 + rng() % 40;
        std::vector<std::vector<std::string>> queries(B);
        const size_t empty_query = rng() % B;
        std::vector<std::string> seen;
        for (size_t i = 0; i < n_terms; ++i) {
            size_t q = rng() % B;
            if (q == empty_query && B > 1) q = (q + 1) % B;
            std::string t = (!seen.empty() && rng() % 4 == 0) ? seen[rng() % seen.size()] : random_term(rng);
            if (!queries[q].empty() && rng() % 16 == 0) t = queries[q][rng() % queries[q].size()];      // twice in one query
            seen.push_back(t);
            queries[q].push_back(t);
        }
        std::vector<std::string> lead;
        for (size_t i = rng() % 5; i > 0; --i) lead.push_back(random_term(rng));
        check_distinct(lead, queries);
        std::map<std::string, int> cnt;
        for (auto &t : seen) repeats += cnt[t]++ > 0;
        ++batches;
    }
    // offsets that decrease at the first, a middle and the last term of the batch: the ABSOLUTE index comes back
    for (uint32_t lead : {0u, 3u}) {
        const std::vector<std::string> q0 = {"aa", "bb", "cc"}, q1 = {"dd", "ee"};
        for (uint32_t bad : {0u, 2u, 4u}) {
            Batch b = make_batch(std::vector<std::string>(lead, "ll"), {q0, q1});
            // term lead + bad ends in front of its start: push the start up (the term before it grows, which is allowed)
            b.term_off[lead + bad] = b.term_off[lead + bad + 1] + 1;
            Distinct d;
            CHECK(distinct_terms(b.pool.data(), b.term_off.data(), b.qoff.data(), b.B, d) == (int64_t)(lead + bad));
        }
    }
    // the table: a power of two, at least 16, at least 2 n + 2
    CHECK(table_size(0) == 16 && table_size(7) == 16 && table_size(8) == 32);
    CHECK(table_size(30) == 64 && table_size(31) == 64 && table_size(32) == 128);
    CHECK(table_size(2047) == 4096 && table_size(2048) == 8192 && table_size(3000) == 8192);
    for (uint32_t n : {31u, 32u}) {                     // ... and a batch of exactly that many distinct terms through it
        std::vector<std::string> q;
        for (uint32_t i = 0; i < n; ++i) q.push_back("t" + std::to_string(i));
        check_distinct({}, {q, q});
    }
}

// ---- the image
static const uint32_t kLens[12] = {0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 100};

static std::string image_term(uint32_t t, std::mt19937_64 &rng)      // distinct by t; bytes above 0x7f among them
{
    uint32_t len = kLens[t % 12];
    if (len == 0 && t >= 12) len = 2;
    std::string s(len, '\0');
    if (len == 1) { s[0] = (char)(1 + t / 12); return s; }            // (t / 12 < 255 for the sizes used)
    for (uint32_t k = 0; k < len; ++k) s[k] = (char)(uint8_t)(rng() | (k % 5 == 4 ? 0x80 : 0));
    if (len >= 2) { s[0] = (char)(t & 0xFF); s[1] = (char)(t >> 8); }
    return s;
}

static void put32(std::vector<uint8_t> &img, size_t at, uint32_t v)
{
    for (int i = 0; i < 4; ++i) img[at + (size_t)i] = (uint8_t)(v >> (8 * i));
}

// what the lookup form's tables hold, from the terms alone: (class, key, term number) ascending, the boundary of class c = the
// entries of the classes in front of it, the Bloom hash restated
static uint32_t oracle_first_dword(const std::string &t)
{
    uint32_t v = 0;
    for (size_t k = 0; k < 4 && k < t.size(); ++k) v |= (uint32_t)(uint8_t)t[k] << (8 * k);
    return v;
}
static uint32_t oracle_bloom_hash(uint32_t key, uint32_t cls)
{
    uint32_t h = (uint32_t)((uint64_t)(key ^ (uint32_t)((uint64_t)cls * 0x9E3779B9ull)) * 2654435761ull);
    h ^= h >> 15;
    return h % (1u << 17);
}
struct OracleTables {
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> order;
    uint32_t lk[8] = {0};
    std::vector<uint32_t> bloom = std::vector<uint32_t>((1u << 17) / 32, 0u);
};
static OracleTables oracle_tables(const std::vector<std::string> &terms)
{
    OracleTables o;
    for (uint32_t t = 0; t < terms.size(); ++t)
        if (terms[t].size() >= 1 && terms[t].size() <= 16)
            o.order.emplace_back((uint32_t)std::min<size_t>(terms[t].size(), 4) - 1, oracle_first_dword(terms[t]), t);
    std::sort(o.order.begin(), o.order.end());
    for (auto &e : o.order) {
        for (uint32_t c = std::get<0>(e) + 1; c <= 4; ++c) o.lk[c] += 1;
        const uint32_t hb = oracle_bloom_hash(std::get<1>(e), std::get<0>(e));
        o.bloom[hb / 32] |= 1u << (hb % 32);
    }
    return o;
}

static void test_image(std::mt19937_64 &rng, long &images, long &bytes_compared)
{
    for (int lookup = 0; lookup <= 1; ++lookup)
        for (uint32_t TT : {1u, 63u, 64u, 65u, 3000u}) {
            std::vector<std::string> terms;
            for (uint32_t t = 0; t < TT; ++t) terms.push_back(image_term(t, rng));
            // queries that together hold every term once in order (so that term t is distinct term t) and repeats behind them
            const size_t B = 1 + rng() % 7;
            std::vector<std::vector<std::string>> queries(B);
            for (uint32_t t = 0; t < TT; ++t) queries[(size_t)t * B / TT].push_back(terms[t]);
            for (size_t i = 0; i < 20; ++i) queries[B - 1].push_back(terms[rng() % TT]);
            const Batch b = make_batch({"lead"}, queries);
            Distinct d;
            CHECK(distinct_terms(b.pool.data(), b.term_off.data(), b.qoff.data(), b.B, d) == -1);
            CHECK(d.terms.size() == TT);
            const uint32_t n_total = b.qoff[B] - b.qoff[0];
            const MetaLayout l = layout_of(TT, n_total, b.B, d.pool_bytes, lookup != 0);
            // the regions: ascending, each where the one in front of it ends, aligned, the last ending at meta_bytes
            const size_t starts[8] = {l.terms, l.qmeta, l.iota, l.match, l.match8, l.lk, l.pool, l.bloom};
            const size_t sizes[7] = {16 * (size_t)TT, 4 * ((size_t)n_total + B + 1), 4 * 65, 48 * (size_t)TT, 80 * (size_t)TT, 4 * (8 + 2 * (size_t)TT), d.pool_bytes + 16};
            CHECK(starts[0] == 0);
            for (int r = 0; r < 6; ++r) CHECK(starts[r + 1] == starts[r] + sizes[r] && starts[r] % 4 == 0);
            CHECK(l.bloom % 16 == 0 && l.bloom >= l.pool + sizes[6] && l.bloom < l.pool + sizes[6] + 16);
            CHECK(l.meta_bytes == (lookup ? l.bloom + (1u << 17) / 8 : l.pool + sizes[6]));
            // the image, byte by byte; what is not written keeps the fill
            std::vector<uint8_t> want(l.meta_bytes, 0xA5);
            size_t cursor = 0;
            for (uint32_t t = 0; t < TT; ++t) {
                const std::string &s = terms[t];
                const uint32_t len = (uint32_t)s.size();
                put32(want, l.terms + 16 * (size_t)t + 0, (uint32_t)cursor);
                put32(want, l.terms + 16 * (size_t)t + 4, len);
                for (size_t k = 0; k < 4; ++k) {
                    want[l.terms + 16 * (size_t)t + 8 + k] = k < len ? (uint8_t)s[k] : 0;
                    want[l.terms + 16 * (size_t)t + 12 + k] = k < len ? 0xFF : 0;
                }
                for (size_t k = 0; k < 16; ++k) {
                    want[l.match + 48 * (size_t)t + k] = k < len ? (uint8_t)s[k] : 0;
                    want[l.match + 48 * (size_t)t + 16 + k] = k < len ? 0xFF : 0;
                }
                put32(want, l.match + 48 * (size_t)t + 32, len);
                for (size_t k = 36; k < 48; ++k) want[l.match + 48 * (size_t)t + k] = 0;
                for (size_t k = 0; k < 32; ++k) {
                    want[l.match8 + 80 * (size_t)t + k] = k < len ? (uint8_t)s[k] : 0;
                    want[l.match8 + 80 * (size_t)t + 32 + k] = k < len ? 0xFF : 0;
                }
                put32(want, l.match8 + 80 * (size_t)t + 64, len);
                for (size_t k = 68; k < 80; ++k) want[l.match8 + 80 * (size_t)t + k] = 0;
                for (size_t k = 0; k < len; ++k) want[l.pool + cursor + k] = (uint8_t)s[k];
                cursor += len;
            }
            CHECK(cursor == d.pool_bytes);
            {
                size_t at = l.qmeta, i = 0;
                for (auto &q : queries)
                    for (auto &t : q) {
                        uint32_t number = 0;
                        while (terms[number] != t) ++number;
                        put32(want, at + 4 * i++, number);
                    }
                uint32_t off = 0;
                for (size_t q = 0; q <= B; ++q) {
                    put32(want, at + 4 * i++, off);
                    if (q < B) off += (uint32_t)queries[q].size();
                }
                CHECK(at + 4 * i == l.iota);
            }
            for (uint32_t i = 0; i < 65; ++i) put32(want, l.iota + 4 * (size_t)i, i);
            if (lookup) {
                const OracleTables o = oracle_tables(terms);
                for (int c = 0; c < 8; ++c) put32(want, l.lk + 4 * (size_t)c, o.lk[c]);
                for (size_t i = 0; i < o.order.size(); ++i) {
                    put32(want, l.lk + 4 * (8 + i), std::get<1>(o.order[i]));
                    put32(want, l.lk + 4 * (8 + (size_t)TT + i), std::get<2>(o.order[i]));
                }
                for (size_t i = 0; i < o.bloom.size(); ++i) put32(want, l.bloom + 4 * i, o.bloom[i]);
                CHECK(o.lk[5] == 0 && o.lk[6] == 0 && o.lk[7] == 0 && o.lk[4] == o.order.size());
            }
            // exactly meta_bytes from malloc: a byte too far is a heap error under the sanitizer
            uint8_t *block = static_cast<uint8_t *>(malloc(l.meta_bytes));
            memset(block, 0xA5, l.meta_bytes);
            fill_meta(block, l, d, lookup != 0);
            size_t first_diff = l.meta_bytes;
            for (size_t i = 0; i < l.meta_bytes; ++i)
                if (block[i] != want[i]) { first_diff = i; break; }
            if (first_diff != l.meta_bytes) fprintf(stderr, "lookup %d TT %u: byte %zu of %zu differs\n", lookup, TT, first_diff, l.meta_bytes);
            CHECK(first_diff == l.meta_bytes);
            free(block);
            ++images;
            bytes_compared += (long)l.meta_bytes;
        }
}

// classes that stay empty inherit the boundary in front of them; ties of (class, key) go by term number
static void test_tables(long &tables)
{
    const std::vector<std::vector<std::string>> sets = {
        {"abcd", "abcdzz", "abcdyy", "q", "abcd1"},                     // one class only, four equal keys
        {"xy", "xy", "abcde", "abcdf"},                                 // classes 1 and 3; the same term twice keeps both numbers
        {"", "seventeen-bytes-xx", "z"},                                // nothing but class 0 qualifies
        {"", "a-term-of-more-than-sixteen-bytes"},                      // an empty table
        {"abc", "ab", "a", "abcd", "b", "bc", "bcd", "bcde"},
    };
    for (auto &terms : sets) {
        const Batch b = make_batch({}, {terms});
        Distinct d;
        d.terms.clear();
        for (auto &t : terms) d.terms.emplace_back(t);                  // as given: fill_meta does not ask for distinct terms
        d.qmeta.assign(terms.size() + 2, 0u);
        d.pool_bytes = 0;
        for (auto &t : terms) d.pool_bytes += t.size();
        const uint32_t TT = (uint32_t)terms.size();
        const MetaLayout l = layout_of(TT, TT, 1, d.pool_bytes, true);
        uint8_t *block = static_cast<uint8_t *>(malloc(l.meta_bytes));
        fill_meta(block, l, d, true);
        const uint32_t *lk = reinterpret_cast<const uint32_t *>(block + l.lk), *keys = lk + 8, *tix = keys + TT;
        const OracleTables o = oracle_tables(terms);
        for (int c = 0; c < 8; ++c) CHECK(lk[c] == o.lk[c]);
        for (int c = 0; c < 4; ++c) CHECK(lk[c] <= lk[c + 1]);
        for (size_t i = 0; i < o.order.size(); ++i) {
            CHECK(keys[i] == std::get<1>(o.order[i]) && tix[i] == std::get<2>(o.order[i]));
            if (i && keys[i] == keys[i - 1] && std::get<0>(o.order[i]) == std::get<0>(o.order[i - 1])) CHECK(tix[i - 1] < tix[i]);
        }
        CHECK(memcmp(block + l.bloom, o.bloom.data(), (1u << 17) / 8) == 0);
        free(block);
        ++tables;
        (void)b;
    }
}

static long test_choices()
{
    long n = 0;
    // short_form: the call's override, then the environment's, then 64 terms and 2^25 pairs
    const int64_t big = (int64_t)1 << 40;
    for (int forced = -1; forced <= 1; ++forced)
        for (int env = -1; env <= 1; ++env) {
            for (uint32_t TT : {1u, 63u, 64u, 3000u})
                for (int64_t V : {(int64_t)0, (int64_t)1, big}) {
                    const bool rule = TT >= 64 && (int64_t)TT * V >= ((int64_t)1 << 25);
                    const bool want = forced >= 0 ? forced == 1 : env >= 0 ? env == 1 : rule;
                    CHECK(short_form(TT, V, forced, env) == want);
                }
            ++n;
        }
    CHECK(!short_form(63, big, -1, -1) && short_form(64, big, -1, -1));
    CHECK(!short_form(64, ((int64_t)1 << 19) - 1, -1, -1) && short_form(64, (int64_t)1 << 19, -1, -1));         // 2^25 - 64, 2^25 pairs
    CHECK(!short_form(((1u << 25) - 1), 1, -1, -1) && short_form(1u << 25, 1, -1, -1));                          // 2^25 - 1, 2^25 pairs
    CHECK(short_form(7, 0, -1, 5) && short_form(7, 0, 5, 0));                                                    // any value but 0 is "on"
    // mid_tokens: the same precedence; never more than the list holds
    for (int forced = -1; forced <= 0; ++forced)
        for (int env_off = 0; env_off <= 1; ++env_off) {
            const bool off = forced >= 0 ? forced == 0 : env_off != 0;
            CHECK(mid_tokens(10, 25, forced, env_off != 0) == (off ? 0 : 10));
            CHECK(mid_tokens(10, 4, forced, env_off != 0) == (off ? 0 : 4));
            CHECK(mid_tokens(0, 4, forced, env_off != 0) == 0 && mid_tokens(3, 0, forced, env_off != 0) == 0);
        }
    CHECK(mid_tokens(10, 25, 1, true) == 10);            // an override that is not "off" wins over the environment's "off"
    return n;
}

static void test_hit_list()
{
    // no tokens: a slot per term all the same (the list is never empty)
    CHECK(hit_list(0, 5, 100).max_hits == 5 && !hit_list(0, 5, 100).overflow_possible);
    CHECK(hit_list(0, 5, 4).max_hits == 4 && hit_list(0, 5, 4).overflow_possible);
    CHECK(hit_list(10, 10, 100).max_hits == 100 && !hit_list(10, 10, 100).overflow_possible);      // at the cap
    CHECK(hit_list(10, 10, 101).max_hits == 100 && !hit_list(10, 10, 101).overflow_possible);
    CHECK(hit_list(10, 10, 99).max_hits == 99 && hit_list(10, 10, 99).overflow_possible);
    CHECK(hit_list((int64_t)1 << 33, 3000, 16u << 20).max_hits == (16u << 20) && hit_list((int64_t)1 << 33, 3000, 16u << 20).overflow_possible);
    CHECK(hit_list((int64_t)1 << 33, 3000, 0xFFFFFFFFu).max_hits == 0xFFFFFFFFu);
    // after_run: stands up to max_hits; beyond it the list grows, up to 8 GiB of hits
    CHECK(after_run(0, 0).kind == AfterRun::Stands && after_run(16, 16).kind == AfterRun::Stands && after_run(15, 16).kind == AfterRun::Stands);
    const AfterRun g = after_run(17, 16);
    CHECK(g.kind == AfterRun::Grow && g.new_cap == 17 + 4 + 1024);
    CHECK(after_run(4000, 16).new_cap == 4000 + 1000 + 1024);
    const uint32_t edge = (uint32_t)((((uint64_t)8 << 30)) / kHitBytes);      // the most hits whose list is not above 8 GiB
    CHECK((uint64_t)edge * kHitBytes <= ((uint64_t)8 << 30) && (uint64_t)(edge + 1) * kHitBytes > ((uint64_t)8 << 30));
    CHECK(after_run(edge, 16).kind == AfterRun::Grow && after_run(edge, 16).new_cap == edge + edge / 4 + 1024u);
    CHECK(after_run(edge + 1, 16).kind == AfterRun::Refused && after_run(0xFFFFFFFFu, 16).kind == AfterRun::Refused);
    CHECK(after_run(edge + 1, edge + 1).kind == AfterRun::Stands);
    CHECK(kMaxRuns == 4 && kHitBytes == 24);
    // a bitmap's words: a bit per row, whole 16-byte vectors
    const int64_t rows[7] = {0, 1, 32, 33, 127, 128, 129}, words[7] = {0, 4, 4, 4, 4, 4, 8};
    for (int i = 0; i < 7; ++i) CHECK(words_per_term(rows[i]) == words[i]);
    CHECK(words_per_term(4101) == 132 && words_per_term((int64_t)1 << 31) == (int64_t)1 << 26);
}

static int dump()
{
    std::string line;
    if (!std::getline(std::cin, line)) return 2;
    const long n = atol(line.c_str());
    std::vector<std::string> terms;
    for (long i = 0; i < n; ++i) {
        if (!std::getline(std::cin, line)) return 2;
        if (line.size() % 2) return 2;
        std::string t;
        for (size_t k = 0; k + 1 < line.size(); k += 2) t.push_back((char)strtoul(line.substr(k, 2).c_str(), nullptr, 16));
        terms.push_back(t);
    }
    const Batch b = make_batch({}, {terms});
    Distinct d;
    if (distinct_terms(b.pool.data(), b.term_off.data(), b.qoff.data(), 1, d) != -1 || d.terms.size() != terms.size()) return 3;   // distinct terms only
    const uint32_t TT = (uint32_t)terms.size();
    const MetaLayout l = layout_of(TT, TT, 1, d.pool_bytes, true);
    uint8_t *block = static_cast<uint8_t *>(malloc(l.meta_bytes));
    fill_meta(block, l, d, true);
    const uint32_t *lk = reinterpret_cast<const uint32_t *>(block + l.lk), *keys = lk + 8, *tix = keys + TT;
    const uint32_t *bloom = reinterpret_cast<const uint32_t *>(block + l.bloom);
    printf("lk");
    for (int c = 0; c < 8; ++c) printf(" %u", lk[c]);
    printf("\nkeys");
    for (uint32_t i = 0; i < lk[4]; ++i) printf(" %u", keys[i]);
    printf("\nterms");
    for (uint32_t i = 0; i < lk[4]; ++i) printf(" %u", tix[i]);
    printf("\nbloom");
    for (uint32_t bit = 0; bit < (uint32_t)orr::kVocabBloomBits; ++bit)
        if ((bloom[bit >> 5] >> (bit & 31)) & 1u) printf(" %u", bit);
    printf("\n");
    free(block);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "--dump") return dump();
    std::mt19937_64 rng(20250219);
    long lists = 0, batches = 0, repeats = 0, images = 0, bytes_compared = 0, tables = 0;
    test_distinct(rng, lists, batches, repeats);
    test_image(rng, images, bytes_compared);
    test_tables(tables);
    const long combos = test_choices();
    test_hit_list();
    printf("exhaustive term lists checked: %ld\n", lists);
    printf("random batches checked: %ld (repeated terms: %ld)\n", batches, repeats);
    printf("images compared: %ld (%ld bytes)\n", images, bytes_compared);
    printf("lookup tables checked: %ld\n", tables);
    printf("forced x env combinations checked: %ld\n", combos);
    if (g_fail) { printf("orr_keyword_plan_selftest: %ld FAILED\n", g_fail); return 1; }
    printf("orr_keyword_plan_selftest: ok\n");
    return 0;
}
