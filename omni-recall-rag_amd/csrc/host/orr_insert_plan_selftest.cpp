// orr_insert_plan_selftest.cpp -- the merge plan of orr_index_insert_rows (orr_insert_plan.h) on the CPU: no HIP, no GPU, no index.
//   orr_insert_plan_selftest <scenario>      exit status 0: the scenario held; 1: a check failed; 2: usage
// tests/test_insert_plan_cpu.py runs every scenario.
//
// Every scenario is a small shard (ticks in candidate order + lowercased contents) and a set of new rows.  The checks:
//   - the merged order equals std::stable_sort by ticks descending over (old rows, then new rows);
//   - plan_sources names, for every destination, the row that order puts there; rows in front of first_moved stay;
//   - the merged token index, read as a map token -> ascending rows, equals build_token_index over the merged contents
//     (vocabulary ORDER may differ), and its pool has the scan kernel's layout;
//   - the deleted positions follow their rows; timestamps zeroed at deleted positions (a loaded shard) are repaired first.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../orr_insert_plan.h"

namespace {

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

struct Rows {
    std::vector<int64_t> ticks;
    std::vector<std::string> text;
    void add(int64_t t, const std::string &s) { ticks.push_back(t); text.push_back(s); }
    size_t size() const { return ticks.size(); }
};

// the rows' contents in the layout build_token_index reads (one pool, starts and lengths)
orr::TokenIndexHost index_of(const std::vector<std::string> &text, int threads = 4)
{
    std::vector<uint8_t> pool;
    std::vector<uint64_t> start;
    std::vector<uint32_t> len;
    for (const auto &s : text) {
        start.push_back(pool.size());
        len.push_back((uint32_t)s.size());
        pool.insert(pool.end(), s.begin(), s.end());
    }
    pool.resize(pool.size() + 16, 0x20);
    orr::TokenIndexHost ti;
    orr::build_token_index(pool.data(), start.data(), len.data(), (int64_t)text.size(), threads, ti);
    return ti;
}

std::map<std::string, std::vector<uint32_t>> as_map(const orr::TokenIndexHost &ti)
{
    std::map<std::string, std::vector<uint32_t>> m;
    CHECK(ti.vstart.size() == ti.vlen.size());
    CHECK(ti.post_off.size() == ti.vstart.size() + 1 || (ti.vstart.empty() && ti.post_off.size() <= 1));
    for (size_t v = 0; v < ti.vstart.size(); ++v) {
        CHECK(ti.vstart[v] % 16 == 0);
        const uint64_t padded = ((uint64_t)ti.vlen[v] / 16 + 1) * 16;
        CHECK(ti.vstart[v] + padded <= ti.vpool.size());
        if (v + 1 < ti.vstart.size()) CHECK(ti.vstart[v + 1] == ti.vstart[v] + padded);
        for (uint64_t i = ti.vlen[v]; i < padded; ++i) CHECK(ti.vpool[ti.vstart[v] + i] == 0x20);      // 1..16 spaces behind it
        std::string tok(reinterpret_cast<const char *>(ti.vpool.data() + ti.vstart[v]), ti.vlen[v]);
        CHECK(!tok.empty() && m.find(tok) == m.end());
        std::vector<uint32_t> rows(ti.post_rows.begin() + ti.post_off[v], ti.post_rows.begin() + ti.post_off[v + 1]);
        CHECK(!rows.empty());
        for (size_t i = 1; i < rows.size(); ++i) CHECK(rows[i - 1] < rows[i]);
        m[tok] = rows;
    }
    if (!ti.post_off.empty()) CHECK(ti.post_off.back() == ti.post_rows.size());
    return m;
}

void check(const Rows &old, const Rows &add, const std::vector<int64_t> &dead = {})
{
    const int64_t n_old = (int64_t)old.size(), n_new = (int64_t)add.size(), n = n_old + n_new;
    for (int64_t p = 1; p < n_old; ++p) CHECK(old.ticks[p - 1] >= old.ticks[p]);     // a sealed shard
    const orr::InsertPlan pl = orr::make_insert_plan(old.ticks.data(), n_old, add.ticks.data(), n_new);

    // reference: what a seal does with old-then-new
    std::vector<int64_t> all_ticks(old.ticks);
    all_ticks.insert(all_ticks.end(), add.ticks.begin(), add.ticks.end());
    std::vector<int64_t> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), (int64_t)0);
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return all_ticks[a] > all_ticks[b]; });

    CHECK(pl.rows() == n && (int64_t)pl.order.size() == n_new && (int64_t)pl.shift.size() == n_old + 1);
    CHECK(pl.shift[(size_t)n_old] == (uint32_t)n_new);
    std::vector<int64_t> src((size_t)n);
    orr::plan_sources(pl, 0, n, src.data());
    for (int64_t d = 0; d < n; ++d) {
        const int64_t want = perm[(size_t)d];
        if (want < n_old) {
            CHECK(src[(size_t)d] == want);
            CHECK(want + pl.shift[(size_t)want] == d);
        } else {
            CHECK(src[(size_t)d] < 0);
            const int64_t k = ~src[(size_t)d];
            CHECK(k >= 0 && k < n_new && pl.order[(size_t)k] == want - n_old && pl.new_pos[(size_t)k] == d);
        }
        if (d < pl.first_moved) CHECK(src[(size_t)d] == d);
    }
    CHECK(pl.first_moved == n_old || src[(size_t)pl.first_moved] < 0);
    // any window of destinations gives the same sources as the whole list (the driver asks chunk by chunk)
    for (int64_t d0 = 0; d0 < n; d0 += 3) {
        const int64_t d1 = std::min<int64_t>(n, d0 + 5);
        std::vector<int64_t> win((size_t)(d1 - d0));
        orr::plan_sources(pl, d0, d1, win.data());
        for (int64_t d = d0; d < d1; ++d) CHECK(win[(size_t)(d - d0)] == src[(size_t)d]);
    }
    const std::vector<int64_t> merged_ticks = orr::merge_rows(pl, old.ticks.data(), add.ticks.data());
    for (int64_t d = 0; d < n; ++d) CHECK(merged_ticks[(size_t)d] == all_ticks[(size_t)perm[(size_t)d]]);

    // deleted rows follow their rows
    const std::vector<int64_t> nd = orr::remap_dead(pl, dead);
    CHECK(nd.size() == dead.size());
    for (size_t i = 0; i < dead.size(); ++i) {
        CHECK(perm[(size_t)nd[i]] == dead[i]);
        if (i) CHECK(nd[i - 1] < nd[i]);
    }

    // token index: the old shard's, the new rows' alone in merged rank order, merged -- against one built from the merged contents
    std::vector<std::string> ranked((size_t)n_new), merged_text((size_t)n);
    for (int64_t k = 0; k < n_new; ++k) ranked[(size_t)k] = add.text[(size_t)pl.order[(size_t)k]];
    for (int64_t d = 0; d < n; ++d) merged_text[(size_t)d] = perm[(size_t)d] < n_old ? old.text[(size_t)perm[(size_t)d]] : add.text[(size_t)(perm[(size_t)d] - n_old)];
    orr::TokenIndexHost ti_old = index_of(old.text), ti_add = index_of(ranked), ti_out;
    ti_old.vpool.resize(ti_old.vpool.size() + 2048, 0x20);                         // the slack the device copy carries
    orr::merge_token_index(ti_old, ti_add, pl, ti_out);
    const auto got = as_map(ti_out), want = as_map(index_of(merged_text));
    CHECK(got == want);
    CHECK(ti_out.vpool.size() == orr::vocab_pool_bytes(ti_out));
    // the old vocabulary keeps its numbers: tokens not seen before are appended
    for (size_t v = 0; v < ti_old.vstart.size(); ++v) CHECK(ti_out.vstart[v] == ti_old.vstart[v] && ti_out.vlen[v] == ti_old.vlen[v]);
}

Rows base_shard()
{
    Rows r;
    const char *words[] = {"alpha", "beta", "gamma delta", "epsilon alpha", "", "zeta beta eta", "theta", "iota kappa alpha"};
    for (int i = 0; i < 40; ++i) r.add(1000 - 10 * (i / 2), std::string(words[i % 8]) + (i % 3 ? " common" : ""));   // pairs of equal ticks
    return r;
}

void front()
{
    Rows add;
    add.add(5000, "alpha newest"); add.add(4000, "brand new tokens"); add.add(6000, "beta");
    check(base_shard(), add);
}

void middle()
{
    Rows add;
    add.add(905, "alpha mid"); add.add(995, "gamma"); add.add(815, "unseen"); add.add(906, "common beta"); add.add(905, "second at 905");
    check(base_shard(), add);
}

void back()
{
    Rows add;
    add.add(1, "oldest alpha"); add.add(0, "older still"); add.add(-5, "negative ticks theta");
    check(base_shard(), add);
}

void ties()
{
    // new rows at the ticks of old rows go BEHIND every old row of that tick and keep their own order
    Rows add;
    add.add(1000, "tie a"); add.add(900, "tie b alpha"); add.add(1000, "tie c"); add.add(810, "tie d"); add.add(900, "tie e");
    check(base_shard(), add);
}

void empty_old()
{
    Rows add;
    add.add(5, "first rows of a shard"); add.add(9, "rows shard"); add.add(5, "of");
    check(Rows(), add);
}

void empty_new()
{
    check(base_shard(), Rows());
    check(Rows(), Rows());
}

void all_equal()
{
    Rows old, add;
    for (int i = 0; i < 9; ++i) old.add(77, "same " + std::to_string(i % 3));
    for (int i = 0; i < 5; ++i) add.add(77, "same new " + std::to_string(i % 2));
    check(old, add);
}

void no_content()
{
    Rows old, add;
    for (int i = 0; i < 6; ++i) old.add(100 - i, i == 2 ? "only one" : "");
    add.add(98, ""); add.add(200, ""); add.add(0, " \t ");
    check(old, add);
    Rows old2;
    for (int i = 0; i < 4; ++i) old2.add(10 - i, "");
    Rows add2;
    add2.add(9, "text arrives"); add2.add(9, "");
    check(old2, add2);                                                             // an old shard without a single token
}

void token_lengths()
{
    // 1, 16, 17, 32, 33 and 200 bytes: the scan kernel's classes (one lane per token up to 32 bytes, a wave beyond) and the pool's padding rule
    const int lens[] = {1, 16, 17, 32, 33, 200};
    Rows old, add;
    int t = 500;
    for (int l : lens) {
        old.add(t--, std::string((size_t)l, 'o') + " shared" + std::to_string(l));
        add.add(t + 3, std::string((size_t)l, 'n') + " " + std::string((size_t)l, 'o'));    // a new token of that length and the old one again
        add.add(1, std::string((size_t)l, 'z'));
    }
    check(old, add);
}

void unicode_whitespace()
{
    // every whitespace character of char.IsWhiteSpace beyond ASCII separates tokens; a lone lead byte does not
    const char *ws[] = {"\xC2\x85", "\xC2\xA0", "\xE1\x9A\x80", "\xE2\x80\x80", "\xE2\x80\x8A", "\xE2\x80\xA8", "\xE2\x80\xA9",
                        "\xE2\x80\xAF", "\xE2\x81\x9F", "\xE3\x80\x80", "\t", "\n", "\x0B", "\x0C", "\r"};
    Rows old, add;
    int t = 100;
    for (const char *w : ws) {
        old.add(t, std::string("left") + w + "right");
        add.add(t, std::string("right") + w + w + "fresh" + w);
        --t;
    }
    add.add(50, "not\xE2\x80\x8Bspace na\xC3\xAFve \xE2\x80");                    // U+200B is no whitespace; a truncated sequence at the end
    old.add(40, "caf\xC3\xA9 \xE6\x97\xA5\xE6\x9C\xAC");
    check(old, add);
}

void deleted_rows()
{
    Rows add;
    add.add(2000, "front"); add.add(950, "mid alpha"); add.add(950, "mid beta"); add.add(900, "tie"); add.add(3, "back");
    check(base_shard(), add, {0, 3, 4, 11, 20, 39});
    check(base_shard(), Rows(), {1, 2});
}

void loaded_tombstones()
{
    // a shard FILE carries the device's timestamps, 0 at every deleted position: the mirror of a loaded shard is repaired
    // before a plan is made from it, so that a new row does not stop at the first deleted row
    {
        std::vector<int64_t> ticks = {10, 9, 0, 7, 6};
        const int64_t add = 5;
        orr::InsertPlan bad = orr::make_insert_plan(ticks.data(), 5, &add, 1);
        CHECK(bad.new_pos[0] == 2);                                                // what the zero does when it is trusted
        orr::repair_dead_ticks(ticks, {2});
        CHECK((ticks == std::vector<int64_t>{10, 9, 9, 7, 6}));
        orr::InsertPlan pl = orr::make_insert_plan(ticks.data(), 5, &add, 1);
        CHECK(pl.new_pos[0] == 5 && pl.first_moved == 5);
    }
    {   // runs of deleted rows, at the very front, at the very end, and everything deleted
        std::vector<int64_t> ticks = {0, 0, 50, 0, 0, 40, 40, 0, 30, 0};
        orr::repair_dead_ticks(ticks, {0, 1, 3, 4, 7, 9});
        CHECK((ticks == std::vector<int64_t>{50, 50, 50, 50, 50, 40, 40, 40, 30, 30}));
        std::vector<int64_t> gone = {0, 0, 0};
        orr::repair_dead_ticks(gone, {0, 1, 2});
        CHECK((gone == std::vector<int64_t>{0, 0, 0}));
        std::vector<int64_t> none = {3, 2, 1};
        orr::repair_dead_ticks(none, {});
        CHECK((none == std::vector<int64_t>{3, 2, 1}));
    }
    // the whole check on a shard whose mirror went through a file: live rows keep their ticks and order, new rows of every age
    Rows old = base_shard();
    const std::vector<int64_t> dead = {0, 1, 7, 8, 9, 20, 38, 39};
    std::vector<int64_t> from_file = old.ticks;
    for (int64_t p : dead) from_file[(size_t)p] = 0;
    orr::repair_dead_ticks(from_file, dead);
    for (size_t p = 1; p < from_file.size(); ++p) CHECK(from_file[p - 1] >= from_file[p]);
    for (size_t p = 0; p < from_file.size(); ++p)
        if (!std::binary_search(dead.begin(), dead.end(), (int64_t)p)) CHECK(from_file[p] == old.ticks[p]);
    old.ticks = from_file;
    Rows add;
    add.add(2000, "front"); add.add(995, "behind the dead front rows"); add.add(960, "mid alpha"); add.add(905, "mid"); add.add(805, "near the end"); add.add(1, "back");
    check(old, add, dead);
    // ... and every new row lands behind every LIVE row that is at least as new, in front of every live row that is older
    const orr::InsertPlan pl = orr::make_insert_plan(old.ticks.data(), (int64_t)old.size(), add.ticks.data(), (int64_t)add.size());
    const Rows truth = base_shard();
    for (size_t k = 0; k < add.size(); ++k) {
        const int64_t t = add.ticks[(size_t)pl.order[k]];
        for (size_t p = 0; p < truth.size(); ++p) {
            if (std::binary_search(dead.begin(), dead.end(), (int64_t)p)) continue;
            const int64_t at = (int64_t)p + pl.shift[p];
            CHECK((truth.ticks[p] >= t) == (at < pl.new_pos[k]));
        }
    }
}

void many_rows()
{
    // a pseudo-random shard large enough for build_token_index to split the rows over threads
    Rows old, add;
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::vector<int64_t> ticks;
    for (int i = 0; i < 9000; ++i) ticks.push_back((int64_t)(rnd() % 3000));
    std::sort(ticks.rbegin(), ticks.rend());
    for (int64_t t : ticks) old.add(t, "w" + std::to_string(rnd() % 500) + " w" + std::to_string(rnd() % 40) + (rnd() % 7 ? "" : " rare" + std::to_string(rnd() % 5000)));
    for (int i = 0; i < 700; ++i) add.add((int64_t)(rnd() % 3200) - 100, "w" + std::to_string(rnd() % 520) + " fresh" + std::to_string(rnd() % 90));
    std::vector<int64_t> dead;
    for (int64_t p = 5; p < 9000; p += 97) dead.push_back(p);
    check(old, add, dead);
}

const struct { const char *name; void (*run)(); } kScenarios[] = {
    {"front", front},
    {"middle", middle},
    {"back", back},
    {"ties", ties},
    {"empty_old", empty_old},
    {"empty_new", empty_new},
    {"all_equal", all_equal},
    {"no_content", no_content},
    {"token_lengths", token_lengths},
    {"unicode_whitespace", unicode_whitespace},
    {"deleted_rows", deleted_rows},
    {"loaded_tombstones", loaded_tombstones},
    {"many_rows", many_rows},
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
    fprintf(stderr, "usage: orr_insert_plan_selftest <scenario>, one of:\n");
    for (const auto &s : kScenarios) fprintf(stderr, "  %s\n", s.name);
    return 2;
}
