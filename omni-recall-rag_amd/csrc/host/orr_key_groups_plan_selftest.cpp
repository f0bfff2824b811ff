// orr_key_groups_plan_selftest -- the rules of the key groups (orr_key_groups_plan.h) on the CPU: the argument order, the sort
// key, the blocks of a run, the slice rule, the finish, and that the blocked sum is its own order -- it differs in bits from a
// plain sequential sum and from a fold of the blocks in reverse on a crafted input.  No HIP, no GPU;
// tests/test_key_groups_cpu.py runs it.
#include "../orr_key_groups_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

using namespace key_groups;

static long g_fail = 0;
#define CHECK(c)                                                                                                                  \
    do {                                                                                                                          \
        if (!(c)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); }                                      \
    } while (0)

static uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
static uint32_t bits_of(float v) { uint32_t b; memcpy(&b, &v, 4); return b; }

static void test_arguments()
{
    CHECK(first_invalid_groups(-1, true, true, true, true, true) == 1);
    CHECK(first_invalid_groups(0, true, true, true, false, true) == 2);
    CHECK(first_invalid_groups(0, true, true, false, true, true) == 2);
    CHECK(first_invalid_groups(5, true, false, false, false, true) == 3);
    CHECK(first_invalid_groups(5, false, true, false, false, true) == 3);
    CHECK(first_invalid_groups(0, true, true, false, false, true) == 4);
    CHECK(first_invalid_groups(5, false, false, false, false, true) == 4);
    CHECK(first_invalid_groups(0, true, true, false, false, false) == 0);
    CHECK(first_invalid_groups(5, false, false, false, false, false) == 0);
    CHECK(first_invalid_centroids(-1, true, true, true) == 1);
    CHECK(first_invalid_centroids(kMaxKeys + 1, false, false, false) == 1);
    CHECK(first_invalid_centroids(3, true, true, true) == 2);
    CHECK(first_invalid_centroids(3, false, true, true) == 3);
    CHECK(first_invalid_centroids(3, false, false, true) == 4);
    CHECK(first_invalid_centroids(0, true, true, true) == 4);
    CHECK(first_invalid_centroids(0, true, true, false) == 0);
    CHECK(first_invalid_centroids(kMaxKeys, false, false, false) == 0);
    CHECK(first_invalid_scope_centroid(true, true) == 1);
    CHECK(first_invalid_scope_centroid(false, true) == 2);
    CHECK(first_invalid_scope_centroid(false, false) == 0);
    CHECK(kBlock == 256 && kCoordsPerPass == 1024 && kMaxKeys == 65536);
}

static void test_sort_key()
{
    const int64_t v[] = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX};
    for (int i = 0; i + 1 < 6; ++i) CHECK(sort_key(v[i]) < sort_key(v[i + 1]));
    for (int i = 0; i < 6; ++i) CHECK(key_of_sort(sort_key(v[i])) == v[i]);
    CHECK(sort_key(INT64_MIN + 1) == 1ull);
    CHECK(sort_key(-1) == 0x7FFFFFFFFFFFFFFFull);
    CHECK(sort_key(0) == 0x8000000000000000ull);
    CHECK(sort_key(INT64_MAX) == 0xFFFFFFFFFFFFFFFFull);
    CHECK(table_bits(1) == 1 && table_bits(2) == 1 && table_bits(3) == 2 && table_bits(2048) == 11 && table_bits(2049) == 12 && table_bits(65536) == 16);
    CHECK(!participates(0.0) && !participates(-0.0) && !participates(-1.0) && !participates(std::nan("")) && participates(1e-300) &&
          participates(INFINITY));
}

static long test_blocks()
{
    long checked = 0;
    const int64_t ns[] = {0, 1, 255, 256, 257, 512, 513, 100000};
    for (int64_t n : ns) {
        std::vector<Block> blocks;
        std::vector<Fold> folds;
        uint32_t next_part = 7;
        blocks_of(n, 1000, 3u, blocks, folds, next_part);
        const int64_t nb = (n + 255) / 256;
        CHECK((int64_t)blocks.size() == nb && n_blocks_of(n) == nb);
        CHECK(folds.size() == (nb > 1 ? 1u : 0u));
        CHECK(next_part == 7u + (nb > 1 ? (uint32_t)nb : 0u));
        if (nb > 1) CHECK(folds[0].slot == 3u && folds[0].part0 == 7u && folds[0].n_blocks == (uint32_t)nb);
        int64_t at = 1000;
        for (int64_t b = 0; b < nb; ++b) {
            const Block &k = blocks[(size_t)b];
            CHECK(k.first == (uint32_t)at && k.slot == 3u && k.index == (uint32_t)b && k.len >= 1 && k.len <= (uint32_t)kBlock);
            CHECK(b + 1 < nb ? k.len == (uint32_t)kBlock : k.len == (uint32_t)(n - b * kBlock));
            CHECK(k.part == (nb > 1 ? 7u + (uint32_t)b : kDirect));
            at += k.len;
            ++checked;
        }
        CHECK(at == 1000 + n);
    }
    // 1,000 members: four blocks of 256, 256, 256 and 232
    std::vector<Block> blocks;
    std::vector<Fold> folds;
    uint32_t next_part = 0;
    blocks_of(1000, 0, 0u, blocks, folds, next_part);
    CHECK(blocks.size() == 4 && blocks[0].len == 256 && blocks[2].len == 256 && blocks[3].len == 232 && next_part == 4);
    return checked;
}

static void test_slices()
{
    CHECK(slice_keys(3072, 0) == 2730);                 // 64 MiB / (8 x 3072)
    CHECK(slice_keys(128, 0) == 65536);                 // capped at the most keys a call lists
    CHECK(slice_keys(70, 0) == 65536);
    CHECK(slice_keys(1 << 24, 0) == 1);                 // never below one key
    CHECK(slice_keys(3072, 1) == 1 && slice_keys(3072, 7) == 7 && slice_keys(128, 65536) == 65536);
    CHECK(slice_keys(3072, -5) == 2730 && slice_keys(3072, 65537) == 2730);
    CHECK(slice_option_valid(0) && slice_option_valid(1) && slice_option_valid(65536) && !slice_option_valid(-1) && !slice_option_valid(65537));
    CHECK((int64_t)slice_keys(3072, 0) * 3072 * 8 <= kSliceBytes);
}

static void test_finish()
{
    // a tie: 1 + 2^-24 lies half way between the floats 1 and 1 + 2^-23 and goes to the even one, 1; the next double above goes up
    const double tie = 1.0 + std::ldexp(1.0, -24);
    double S[3] = {tie * 3.0, std::nextafter(tie, 2.0) * 4.0, -0.0};
    float c[3];
    finish(S, 3, 1, c);
    CHECK(S[0] / 3.0 == tie && bits_of(c[0]) == bits_of(1.0f));
    finish(S + 1, 4, 1, c + 1);
    CHECK(bits_of(c[1]) == bits_of(std::nextafter(1.0f, 2.0f)));
    finish(S + 2, 5, 1, c + 2);
    CHECK(bits_of(c[2]) == 0x80000000u);               // -0.0 / 5 = -0.0: the sign is the sum's
    float z[2] = {7.f, 7.f};
    const double any[2] = {123.0, -4.0};
    finish(any, 0, 2, z);
    CHECK(bits_of(z[0]) == 0u && bits_of(z[1]) == 0u);
    double S0[2] = {7.0, 7.0};
    sum_blocked(nullptr, 2, nullptr, 0, S0);
    CHECK(bits_of(S0[0]) == 0ull && bits_of(S0[1]) == 0ull);
}

// the blocked order against the two orders a wrong kernel would most likely take
static void test_order()
{
    // 600 rows of one coordinate: three blocks of 256, 256 and 88.  Block 0 sums to 2^60 exactly; blocks 1 and 2 hold small values
    // that vanish one by one beside 2^60 (the plain sequential sum) but not as block sums; block 2 carries -2^59, so the reverse
    // fold adds the small block sums in another order.
    const int n = 600;
    std::vector<float> e((size_t)n);
    std::vector<int64_t> member((size_t)n);
    std::iota(member.begin(), member.end(), 0);
    for (int i = 0; i < n; ++i) e[(size_t)i] = 0.f;
    e[0] = std::ldexp(1.f, 60);
    for (int i = 256; i < 512; ++i) e[(size_t)i] = 1.f + (float)(i % 7) * 0.125f;
    for (int i = 512; i < n; ++i) e[(size_t)i] = 3.f + (float)(i % 5) * 0.25f;
    e[512] = -std::ldexp(1.f, 59);
    e[599] = 1e-3f;
    double blocked = 0.0;
    sum_blocked(e.data(), 1, member.data(), n, &blocked);
    volatile double seq = +0.0;
    for (int i = 0; i < n; ++i) seq = seq + (double)e[(size_t)i];
    volatile double P[3] = {+0.0, +0.0, +0.0};
    for (int i = 0; i < n; ++i) P[i / 256] = P[i / 256] + (double)e[(size_t)i];
    volatile double rev = +0.0;
    for (int b = 2; b >= 0; --b) rev = rev + P[b];
    volatile double fwd = +0.0;
    for (int b = 0; b < 3; ++b) fwd = fwd + P[b];
    CHECK(bits_of(blocked) == bits_of((double)fwd));
    CHECK(bits_of(blocked) != bits_of((double)seq));
    CHECK(bits_of(blocked) != bits_of((double)rev));
    // members are taken through their positions, rows through dim
    const float rows[6] = {1.f, 10.f, 2.f, 20.f, 4.f, 40.f};
    const int64_t pick[2] = {2, 0};
    double S[2];
    sum_blocked(rows, 2, pick, 2, S);
    CHECK(S[0] == 5.0 && S[1] == 50.0);
    // a sum started at +0.0 is never -0.0
    const float neg[2] = {-0.f, -0.f};
    const int64_t both[2] = {0, 1};
    sum_blocked(neg, 1, both, 2, S);
    CHECK(bits_of(S[0]) == 0ull);
}

int main()
{
    test_arguments();
    test_sort_key();
    const long blocks = test_blocks();
    test_slices();
    test_finish();
    test_order();
    printf("block records checked: %ld\n", blocks);
    if (g_fail) { printf("orr_key_groups_plan_selftest: %ld FAILED\n", g_fail); return 1; }
    printf("orr_key_groups_plan_selftest: ok\n");
    return 0;
}
