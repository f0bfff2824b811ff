// orr_centroid_index_plan_selftest -- the rules of the document index (orr_centroid_index_plan.h) on the CPU: the argument order,
// the merge of the participating runs into the list of all keys, which keys of a slice are kept, their destination rows, the
// slice walk, the shared finish expression, the slice rule of orr_index_get_rows.  No HIP, no GPU;
// tests/test_centroid_index_cpu.py runs it.
//
// With arguments `walk IN OUT` it is a driver for that test's own restatement: IN holds int64 T, per_slice, used[T], first[T];
// OUT receives int64 n_slices and per slice key0, n_keys, row0, n_kept and n_kept triples (slot, n, first).
#include "../orr_centroid_index_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace centroid_index;

static long g_fail = 0;
#define CHECK(c)                                                                                                                  \
    do {                                                                                                                          \
        if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); }                                      \
    } while (0)

static uint32_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

static void test_arguments()
{
    CHECK(first_invalid(true, true) == 1);
    CHECK(first_invalid(true, false) == 1);
    CHECK(first_invalid(false, true) == 2);
    CHECK(first_invalid(false, false) == 0);
    CHECK(first_invalid_get_rows(-1, true, true, true) == 1);
    CHECK(first_invalid_get_rows(3, true, false, true) == 2);
    CHECK(first_invalid_get_rows(3, false, true, true) == 2);
    CHECK(first_invalid_get_rows(3, false, false, true) == 3);
    CHECK(first_invalid_get_rows(0, true, true, true) == 3);
    CHECK(first_invalid_get_rows(0, true, true, false) == 0);
    CHECK(first_invalid_get_rows(3, false, false, false) == 0);
    CHECK(kept(1) && kept(1000) && !kept(0));
    CHECK(sizeof(Kept) == 12);
}

static void test_merge()
{
    const uint64_t all[] = {1, 5, 9, 12, 40, 41};
    std::vector<int64_t> used, first;
    {   // the runs of keys 5, 12 and 41: the others have no participating member
        const uint64_t rk[] = {5, 12, 41};
        const uint32_t rl[] = {3, 1, 300};
        CHECK(merge_runs(all, 6, rk, rl, 3, 304, used, first));
        const int64_t want_used[] = {0, 3, 0, 1, 0, 300}, want_first[] = {0, 0, 0, 3, 0, 4};
        for (int i = 0; i < 6; ++i) CHECK(used[(size_t)i] == want_used[i] && first[(size_t)i] == want_first[i]);
        CHECK(!merge_runs(all, 6, rk, rl, 3, 303, used, first));        // the runs hold more pairs than there are
        CHECK(!merge_runs(all, 6, rk, rl, 3, 305, used, first));        // ... and fewer
    }
    {   // a run of a key that is not listed; a run of no pair; runs out of order
        const uint64_t rk[] = {5, 13};
        const uint32_t rl[] = {3, 1};
        CHECK(!merge_runs(all, 6, rk, rl, 2, 4, used, first));
        const uint32_t rz[] = {3, 0};
        const uint64_t rk2[] = {5, 12};
        CHECK(!merge_runs(all, 6, rk2, rz, 2, 3, used, first));
        const uint64_t rk3[] = {12, 5};
        CHECK(!merge_runs(all, 6, rk3, rl, 2, 4, used, first));
    }
    CHECK(merge_runs(all, 6, nullptr, nullptr, 0, 0, used, first));     // no key participates: every key is skipped
    for (int i = 0; i < 6; ++i) CHECK(used[(size_t)i] == 0);
    CHECK(merge_runs(nullptr, 0, nullptr, nullptr, 0, 0, used, first) && used.empty());
}

static void test_walk()
{
    //                     slice 0      slice 1      slice 2 (all skipped)   slice 3
    const int64_t used[] = {2, 0, 7,     1, 300, 0,   0, 0, 0,                0, 5};
    const int64_t first[] = {0, 0, 2,    9, 10, 0,    0, 0, 0,                0, 310};
    const std::vector<Slice> w = walk(used, 11, 3);
    CHECK(w.size() == 4);
    const int64_t key0[] = {0, 3, 6, 9}, row0[] = {0, 2, 4, 4};
    const int32_t n_keys[] = {3, 3, 3, 2}, n_kept[] = {2, 2, 0, 1};
    for (size_t i = 0; i < w.size() && i < 4; ++i)
        CHECK(w[i].key0 == key0[i] && w[i].n_keys == n_keys[i] && w[i].row0 == row0[i] && w[i].n_kept == n_kept[i]);
    // the boundary between slices 0 and 1 lies between two kept keys (2 and 3): rows 1 and 2 of the result
    std::vector<Kept> k;
    CHECK(slice_kept(used, first, 0, 3, k) == 2 && k.size() == 2);
    CHECK(k[0].slot == 0 && k[0].n == 2 && k[0].first == 0 && k[1].slot == 2 && k[1].n == 7 && k[1].first == 2);     // slot 1 is skipped: no gap in the rows
    k.clear();
    CHECK(slice_kept(used, first, 3, 3, k) == 2 && k[0].slot == 0 && k[0].first == 9 && k[1].slot == 1 && k[1].n == 300);
    k.clear();
    CHECK(slice_kept(used, first, 6, 3, k) == 0 && k.empty());
    CHECK(slice_kept(used, first, 9, 2, k) == 1 && k[0].slot == 1 && k[0].n == 5 && k[0].first == 310);
    // every slice size gives the same rows: the kept keys in key order, numbered without a gap
    for (int32_t per = 1; per <= 12; ++per) {
        int64_t row = 0, keys = 0;
        for (const Slice &s : walk(used, 11, per)) {
            CHECK(s.key0 == keys && s.row0 == row && s.n_keys >= 1 && s.n_keys <= per);
            std::vector<Kept> kk;
            CHECK(slice_kept(used, first, s.key0, s.n_keys, kk) == s.n_kept);
            for (const Kept &e : kk) CHECK(used[s.key0 + e.slot] == (int64_t)e.n && first[s.key0 + e.slot] == (int64_t)e.first);
            row += s.n_kept;
            keys += s.n_keys;
        }
        CHECK(row == 5 && keys == 11);
    }
    CHECK(walk(used, 0, 5).empty());
    CHECK(walk(used, 11, 65536).size() == 1);
}

static void test_finish_and_slices()
{
    // finish_one is the expression of key_groups::finish
    const double S[] = {1.0, -3.0, 1e300, 0.1, INFINITY, 5e-324};
    for (int64_t n : {(int64_t)1, (int64_t)3, (int64_t)255, (int64_t)1000000}) {
        float c[6];
        key_groups::finish(S, n, 6, c);
        for (int d = 0; d < 6; ++d) CHECK(bits_of(c[d]) == bits_of(key_groups::finish_one(S[d], n)) && bits_of(c[d]) == bits_of((float)(S[d] / (double)n)));
    }
    // a division in fp32 gives other bits: the data that tells them apart
    CHECK(bits_of(key_groups::finish_one(16777219.0, 7)) != bits_of((float)16777219.0 / (float)7));
    CHECK(get_rows_slice(3072) == 5461 && get_rows_slice(1) == (int64_t)16 << 20 && get_rows_slice(0) == (int64_t)16 << 20);
    CHECK(get_rows_slice(1 << 30) == 1);
    CHECK(key_groups::slice_keys(3072, 0) == 2730 && key_groups::slice_keys(8, 0) == key_groups::kMaxKeys);
}

static int drive_walk(const char *in, const char *out)
{
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    int64_t T = 0, per = 0;
    std::vector<int64_t> used, first;
    bool ok = fread(&T, 8, 1, f) == 1 && fread(&per, 8, 1, f) == 1 && T >= 0 && per >= 1;
    if (ok) {
        used.resize((size_t)T);
        first.resize((size_t)T);
        ok = T == 0 || (fread(used.data(), 8, (size_t)T, f) == (size_t)T && fread(first.data(), 8, (size_t)T, f) == (size_t)T);
    }
    fclose(f);
    if (!ok) return 2;
    FILE *o = fopen(out, "wb");
    if (!o) return 2;
    const std::vector<Slice> w = walk(used.data(), T, (int32_t)per);
    const int64_t n = (int64_t)w.size();
    ok = fwrite(&n, 8, 1, o) == 1;
    for (const Slice &s : w) {
        std::vector<Kept> k;
        slice_kept(used.data(), first.data(), s.key0, s.n_keys, k);
        const int64_t head[4] = {s.key0, s.n_keys, s.row0, s.n_kept};
        ok = ok && fwrite(head, 8, 4, o) == 4;
        for (const Kept &e : k) {
            const int64_t t[3] = {e.slot, e.n, e.first};
            ok = ok && fwrite(t, 8, 3, o) == 3;
        }
    }
    ok = fclose(o) == 0 && ok;
    return ok ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "walk") == 0) return drive_walk(argv[2], argv[3]);
    test_arguments();
    test_merge();
    test_walk();
    test_finish_and_slices();
    if (g_fail) { fprintf(stderr, "orr_centroid_index_plan_selftest: %ld failures\n", g_fail); return 1; }
    printf("orr_centroid_index_plan_selftest: ok\n");
    return 0;
}
