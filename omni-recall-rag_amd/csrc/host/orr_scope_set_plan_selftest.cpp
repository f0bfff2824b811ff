// orr_scope_set_plan_selftest -- the rules of orr_scope_set_plan.h on the CPU (no HIP, no GPU): the positions of a time window
// against a row-by-row restatement (ties at both borders, a window inside a run of ties, empty and inverted windows, the int64
// extremes), the range word masks and the combine against single bits, the remap of a bitmap through a move of rows against a
// bit-by-bit restatement (word, 128-row and 32,768-row borders, negative sources, `first` in mid-word), and n_clip_all.
// Exit status 0 and a last line "orr_scope_set_plan_selftest: ok" when everything holds; tests/test_scope_handle_cpu.py runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <random>
#include <vector>

#include "../orr_scope_set_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

using L = std::initializer_list<int64_t>;
static std::pair<int64_t, int64_t> pr(int64_t a, int64_t b) { return {a, b}; }
constexpr int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();

// the rows a window holds, one by one (to == INT64_MAX is the open end)
static std::vector<int64_t> rows_in_window(const std::vector<int64_t> &t, int64_t from, int64_t to)
{
    std::vector<int64_t> out;
    if (from >= to) return out;
    for (size_t p = 0; p < t.size(); ++p)
        if (t[p] >= from && (t[p] < to || to == kMax)) out.push_back((int64_t)p);
    return out;
}

static void check_window(const std::vector<int64_t> &t, int64_t from, int64_t to)
{
    const auto r = scope_set::ticks_range(t.data(), (int64_t)t.size(), from, to);
    const std::vector<int64_t> want = rows_in_window(t, from, to);
    CHECK(r.first >= 0 && r.first <= r.second && r.second <= (int64_t)t.size());
    CHECK(r.second - r.first == (int64_t)want.size());
    if (!want.empty()) CHECK(r.first == want.front() && r.second == want.back() + 1);
}

static void test_ticks_range()
{
    // descending, with runs of equal ticks: 900 x3, 700 x5, 500 x1, 300 x4, 100 x2
    std::vector<int64_t> t;
    for (auto run : {std::pair<int64_t, int>{900, 3}, {700, 5}, {500, 1}, {300, 4}, {100, 2}})
        for (int i = 0; i < run.second; ++i) t.push_back(run.first);
    const int64_t n = (int64_t)t.size();
    for (int64_t from : L{kMin, 0, 100, 101, 299, 300, 301, 500, 700, 701, 900, 901, kMax})
        for (int64_t to : L{kMin, 0, 100, 101, 300, 301, 500, 501, 700, 701, 900, 901, kMax}) check_window(t, from, to);
    // borders ON runs: the lower border takes the whole run, the upper border leaves the whole run out (half-open)
    CHECK(scope_set::ticks_range(t.data(), n, 300, 700) == pr(8, 13));
    CHECK(scope_set::ticks_range(t.data(), n, 300, 701) == pr(3, 13));
    // adjacent windows tile
    const auto a = scope_set::ticks_range(t.data(), n, 100, 500), b = scope_set::ticks_range(t.data(), n, 500, 901);
    CHECK(b.second == a.first && b.first == 0 && a.second == n);
    // a window inside a run of ties holds the run or nothing
    CHECK(scope_set::ticks_range(t.data(), n, 700, 701) == pr(3, 8));
    const auto e = scope_set::ticks_range(t.data(), n, 701, 702);
    CHECK(e.first == e.second);
    // empty and inverted windows, the open ends
    const auto inv = scope_set::ticks_range(t.data(), n, 700, 300), same = scope_set::ticks_range(t.data(), n, 300, 300);
    CHECK(inv.first == inv.second && same.first == same.second);
    CHECK(scope_set::ticks_range(t.data(), n, kMin, kMax) == pr(0, n));
    CHECK(scope_set::ticks_range(t.data(), 0, kMin, kMax) == pr(0, 0));
    // rows AT the extremes: INT64_MAX as `to` is the open end and keeps them, INT64_MIN as `from` keeps the oldest
    std::vector<int64_t> x = {kMax, kMax, 5, kMin, kMin};
    for (int64_t from : L{kMin, kMin + 1, 5, 6, kMax - 1, kMax})
        for (int64_t to : L{kMin, kMin + 1, 5, 6, kMax - 1, kMax}) check_window(x, from, to);
    CHECK(scope_set::ticks_range(x.data(), 5, kMin, kMax) == pr(0, 5));
    CHECK(scope_set::ticks_range(x.data(), 5, kMin, kMax - 1) == pr(2, 5));
    // random corpora with many ties against the restatement
    std::mt19937_64 rng(7);
    for (int rep = 0; rep < 200; ++rep) {
        std::vector<int64_t> r((size_t)(rng() % 70));
        for (auto &v : r) v = (int64_t)(rng() % 12);
        std::sort(r.begin(), r.end(), std::greater<int64_t>());
        for (int64_t from = -1; from <= 12; ++from)
            for (int64_t to = -1; to <= 13; ++to) check_window(r, from, to);
    }
}

static void test_range_word_and_combine()
{
    for (int64_t p0 : L{0, 1, 31, 32, 33, 63, 64, 70, 127, 128, 160})
        for (int64_t p1 : L{0, 1, 31, 32, 33, 63, 64, 70, 127, 128, 160})
            for (int64_t w = 0; w < 5; ++w) {
                uint32_t want = 0;
                for (int b = 0; b < 32; ++b)
                    if (w * 32 + b >= p0 && w * 32 + b < p1) want |= 1u << b;
                CHECK(scope_set::range_word(w, p0, p1) == want);
            }
    std::mt19937 rng(3);
    for (int rep = 0; rep < 1000; ++rep) {
        const uint32_t a = rng(), b = rng();
        for (int32_t op = 0; op < 3; ++op) {
            uint32_t want = 0;
            for (int i = 0; i < 32; ++i) {
                const bool x = (a >> i) & 1u, y = (b >> i) & 1u;
                const bool z = op == scope_set::And ? (x && y) : op == scope_set::Or ? (x || y) : (x && !y);
                want |= (uint32_t)z << i;
            }
            CHECK(scope_set::combine_word(a, b, op) == want);
        }
    }
    CHECK(scope_set::op_valid(0) && scope_set::op_valid(2) && !scope_set::op_valid(-1) && !scope_set::op_valid(3));
    CHECK(scope_set::scopes_valid(1) && scope_set::scopes_valid(64) && !scope_set::scopes_valid(0) && !scope_set::scopes_valid(65));
}

static int64_t words_for(int64_t rows) { return ((std::max<int64_t>(rows, 1) + 31) / 32 + 3) / 4 * 4; }     // scope::bitmap_bytes / 4

// A move of rows given by `first` and its source list (compaction: the live positions; insertion: new rows are negative):
// the expected scope is followed row by row, the bitmap goes through remap_word.
static void check_remap(int64_t n_old, const std::vector<uint8_t> &in_scope, const std::vector<int64_t> &src, int64_t first)
{
    const int64_t n_new = first + (int64_t)src.size();
    const int64_t ow = words_for(n_old), nw = words_for(n_new);
    std::vector<uint32_t> old_bm((size_t)ow, 0u);
    for (int64_t p = 0; p < n_old; ++p)
        if (in_scope[(size_t)p]) old_bm[(size_t)(p >> 5)] |= 1u << (p & 31);
    for (int64_t w = 0; w < nw; ++w) {
        const uint32_t got = scope_set::remap_word(old_bm.data(), ow, w, first, n_new, src.data());
        for (int b = 0; b < 32; ++b) {
            const int64_t d = w * 32 + b;
            bool want = false;
            if (d < first) want = in_scope[(size_t)d];
            else if (d < n_new && src[(size_t)(d - first)] >= 0) want = in_scope[(size_t)src[(size_t)(d - first)]];
            if ((((got >> b) & 1u) != 0u) != want) { CHECK(!"remap_word differs from the row-by-row move"); return; }
        }
    }
}

static void test_remap()
{
    std::mt19937_64 rng(11);
    for (int64_t n_old : L{1, 31, 32, 33, 127, 128, 129, 1000, 32767, 32768, 32769, 70001}) {
        std::vector<uint8_t> in((size_t)n_old);
        for (auto &v : in) v = (uint8_t)(rng() % 3 == 0);
        in[0] = 1; in[(size_t)n_old - 1] = 1;
        // compaction: first = 0, the sources are the live positions; rows at every border go
        {
            std::vector<int64_t> live;
            for (int64_t p = 0; p < n_old; ++p) {
                const bool dead = p == 0 || p == n_old - 1 || (p >= 128 && p < 256) || p == 32767 || p == 32768 || rng() % 9 == 0;
                if (!dead) live.push_back(p);
            }
            check_remap(n_old, in, live, 0);
        }
        // insertion: new rows (negative sources ~k) in front, through the middle and behind, `first` wherever the first one lands
        for (int64_t first : L{0, 5, 31, 32, 45, 127, 128, 32760, 32768, n_old}) {
            if (first > n_old) continue;
            std::vector<int64_t> src;
            int64_t p = first, k = 0;
            src.push_back(~(k++));                                           // the row at `first` is new (that is what makes it `first`)
            while (p < n_old) {
                if (rng() % 40 == 0 || p == 32767 || p == 127) src.push_back(~(k++));
                src.push_back(p++);
            }
            for (int i = 0; i < 40; ++i) src.push_back(~(k++));              // behind the last old row, across a word border
            check_remap(n_old, in, src, first);
        }
    }
    // bits at or above the new row count and the padding words are zero even when the old bitmap was full
    {
        const int64_t n_old = 200, ow = words_for(n_old);
        std::vector<uint32_t> full((size_t)ow, 0xFFFFFFFFu);
        std::vector<int64_t> src(100);
        for (int64_t i = 0; i < 100; ++i) src[(size_t)i] = i * 2;
        const int64_t nw = words_for(100);
        for (int64_t w = 0; w < nw; ++w)
            CHECK(scope_set::remap_word(full.data(), ow, w, 0, 100, src.data()) == scope_set::range_word(w, 0, 100));
    }
}

static void test_n_clip_all()
{
    constexpr int32_t kChunkWords = 1024;
    std::mt19937_64 rng(5);
    for (int64_t rows : L{1, 32, 100, 32768, 32769, 70001, 100000}) {
        const int64_t words = words_for(rows);
        const int32_t n_chunks = (int32_t)((words + kChunkWords - 1) / kChunkWords);
        for (int rep = 0; rep < 20; ++rep) {
            std::vector<uint32_t> bm((size_t)words, 0u), cc((size_t)n_chunks, 0u);
            int64_t last = -1;
            const int n_set = rep == 0 ? 0 : (int)(rng() % 5) + 1;
            for (int i = 0; i < n_set; ++i) {
                const int64_t p = rep == 1 ? rows - 1 : rep == 2 ? 0 : (int64_t)(rng() % (uint64_t)rows);
                if (!((bm[(size_t)(p >> 5)] >> (p & 31)) & 1u)) { bm[(size_t)(p >> 5)] |= 1u << (p & 31); cc[(size_t)((p >> 5) / kChunkWords)] += 1; }
                last = std::max(last, p);
            }
            CHECK(scope_set::n_clip_all(bm.data(), words, cc.data(), n_chunks, kChunkWords) == last + 1);
        }
    }
}

int main()
{
    test_ticks_range();
    test_range_word_and_combine();
    test_remap();
    test_n_clip_all();
    if (g_failed) { printf("orr_scope_set_plan_selftest: %d check(s) FAILED\n", g_failed); return 1; }
    printf("orr_scope_set_plan_selftest: ok\n");
    return 0;
}
