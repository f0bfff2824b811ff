// orr_keyword_plan.h -- the host half of the keyword chain of a hybrid batch (orr_api.hip: launch_keyword_side), as plain
// functions: what the chain uploads and how large its hit list is, decided before anything is launched.
//
//   distinct terms  the batch's terms (queries b = 0 .. B-1 own terms qoff[b] .. qoff[b+1] of term_off) in order of FIRST
//                   APPEARANCE -- that order numbers the term bitmaps -- found by open addressing on an FNV-1a hash of the bytes;
//                   per term of the batch its distinct number, per query its offset relative to the batch's first term.
//   the image       one pinned block, one upload, eight regions (layout_of): [ScanTerm x TT][term -> distinct number][B + 1 query
//                   offsets][iota 0..64][MatchTerm x TT][MatchTerm8 x TT][lk: 8 class boundaries, TT keys, TT term numbers]
//                   [term bytes + 16 bytes of slack][Bloom bits, 16-byte aligned: the lookup form only].  fill_meta writes it.
//   lookup tables   the terms of 1 .. 16 bytes sorted by (class = min(bytes, 4) - 1, length-masked first dword, term number);
//                   lk[c] .. lk[c + 1] is class c's run in keys / term numbers, an empty class inherits the boundary in front of
//                   it, lk[5..7] = 0; bit vocab_bloom_hash(key, class) of the Bloom filter is set for every entry.
//   short_form      tokens of at most 16 bytes: every (token, term) pair compared (false) or the terms looked up (true).  A
//                   per-call override first, then the environment's, then: at least 64 terms and 2^25 pairs.
//   mid_tokens      how many tokens of 17 .. 32 bytes go through the lane-per-token kernel: all of them unless switched off.
//   the hit list    hit_list: max(tokens, 1) x TT (token, term) pairs at most, cut at the lane's cap -- then the list may prove too
//                   short.  after_run: a run whose hits fit stands; else the list grows to the measured count, a quarter more
//                   and 1024, and the chain runs again -- unless that many hits (kHitBytes each) are more than 8 GiB: refused.
//                   kMaxRuns runs at most.
//
// Host-only C++17, no HIP include (vocab_bloom_hash is __host__ __device__ under hipcc: the lookup kernel shares it);
// host/orr_keyword_plan_selftest.cpp checks all of it on a machine without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string_view>
#include <utility>
#include <vector>

namespace orr {

// Per-term metadata for the keyword scan (built on the host per batch).
struct ScanTerm {
    uint32_t off;      // byte offset of the term in the term pool
    uint32_t len;      // bytes
    uint32_t prefix;   // first min(4,len) bytes, little-endian packed
    uint32_t mask;     // byte mask of those bytes
};

// A query term for the lane-per-token matcher: its first 16 bytes as dwords with byte masks.
struct MatchTerm {
    uint32_t w[4], m[4];
    uint32_t len;       // bytes; terms longer than 16 bytes cannot occur in the tokens this kernel covers
    uint32_t pad[3];
};
struct MatchTerm8 {                   // the same with eight dwords: terms of up to 32 bytes against tokens of 17..32 bytes
    uint32_t w[8], m[8];
    uint32_t len;
    uint32_t pad[3];
};

// bloom: kVocabBloomBits bits, bit vocab_bloom_hash(key, class) set for every (class, key) of the lookup tables.
constexpr int kVocabBloomBits = 1 << 17;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t vocab_bloom_hash(uint32_t key, uint32_t cls)
{
    uint32_t h = (key ^ (cls * 0x9E3779B9u)) * 2654435761u;
    h ^= h >> 15;
    return h & (uint32_t)(kVocabBloomBits - 1);
}

}  // namespace orr

namespace keyword {

// 32-bit words of one term's row bitmap: a bit per row, rounded up to 16 bytes
inline int64_t words_per_term(int64_t n_rows) { return ((n_rows + 31) / 32 + 3) / 4 * 4; }

// ---- the distinct terms of a batch
struct Distinct {
    std::vector<std::string_view> terms;   // in order of first appearance
    std::vector<uint32_t> qmeta;           // [term of the batch -> distinct number][B + 1 query offsets, relative to the first term]
    size_t pool_bytes = 0;                 // bytes of the distinct terms together
};

inline uint32_t table_size(uint32_t n_terms_total)      // slots of the open-addressing table: a power of two, at most half full
{
    uint32_t size = 16;
    while (size < 2 * n_terms_total + 2) size <<= 1;
    return size;
}

// -1, or the ABSOLUTE index of the first term whose offsets decrease (out is then unspecified).  qoff: B + 1 entries.
inline int64_t distinct_terms(const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *qoff, int32_t B, Distinct &out)
{
    const uint32_t t_begin = qoff[0], n_terms_total = qoff[(size_t)B] - qoff[0];
    out.terms.clear();
    out.terms.reserve(n_terms_total);
    const uint32_t size = table_size(n_terms_total);
    std::vector<uint32_t> table(size, 0xFFFFFFFFu);
    out.qmeta.resize((size_t)n_terms_total + (size_t)B + 1);
    for (uint32_t t = 0; t < n_terms_total; ++t) {
        const uint32_t o = term_off[t_begin + t], e = term_off[t_begin + t + 1];
        if (e < o) return (int64_t)t_begin + t;
        std::string_view sv(reinterpret_cast<const char *>(terms_utf8) + o, e - o);
        uint64_t h = 1469598103934665603ull;
        for (unsigned char ch : sv) h = (h ^ ch) * 1099511628211ull;
        uint32_t slot = (uint32_t)(h ^ (h >> 32)) & (size - 1);
        while (table[slot] != 0xFFFFFFFFu && out.terms[table[slot]] != sv) slot = (slot + 1) & (size - 1);
        if (table[slot] == 0xFFFFFFFFu) {
            table[slot] = (uint32_t)out.terms.size();
            out.terms.push_back(sv);
        }
        out.qmeta[t] = table[slot];
    }
    for (int32_t b = 0; b <= B; ++b) out.qmeta[n_terms_total + b] = qoff[b] - t_begin;
    out.pool_bytes = 0;
    for (auto &d : out.terms) out.pool_bytes += d.size();
    return -1;
}

// ---- the image
struct MetaLayout {
    size_t terms, qmeta, iota, match, match8, lk, pool, bloom;   // byte offsets of the regions, ascending
    size_t meta_bytes;                                           // what is reserved and uploaded
};
constexpr size_t kIota = 65, kLkHead = 8, kPoolSlack = 16;

inline MetaLayout layout_of(uint32_t TT, uint32_t n_terms_total, int32_t B, size_t pool_bytes, bool lookup)
{
    // every region in front of the term bytes is made of dwords and starts at a multiple of four; the Bloom bits are read as uint4
    static_assert(alignof(orr::ScanTerm) == 4 && sizeof(orr::ScanTerm) % 4 == 0, "ScanTerm region");
    static_assert(alignof(orr::MatchTerm) == 4 && sizeof(orr::MatchTerm) % 4 == 0, "MatchTerm region");
    static_assert(alignof(orr::MatchTerm8) == 4 && sizeof(orr::MatchTerm8) % 4 == 0, "MatchTerm8 region");
    static_assert(alignof(uint32_t) == 4 && orr::kVocabBloomBits % (8 * 16) == 0, "qmeta, iota, lk and Bloom regions");
    MetaLayout l;
    l.terms = 0;
    l.qmeta = l.terms + sizeof(orr::ScanTerm) * TT;
    l.iota = l.qmeta + sizeof(uint32_t) * ((size_t)n_terms_total + (size_t)B + 1);
    l.match = l.iota + sizeof(uint32_t) * kIota;
    l.match8 = l.match + sizeof(orr::MatchTerm) * TT;
    l.lk = l.match8 + sizeof(orr::MatchTerm8) * TT;
    l.pool = l.lk + sizeof(uint32_t) * (kLkHead + 2 * (size_t)TT);
    l.bloom = (l.pool + pool_bytes + kPoolSlack + 15) / 16 * 16;
    l.meta_bytes = lookup ? l.bloom + orr::kVocabBloomBits / 8 : l.pool + pool_bytes + kPoolSlack;
    return l;
}

// The whole image into `block` (meta_bytes of it, 16-byte aligned).  The pool's slack is not written, and without `lookup`
// neither the lk region nor the Bloom bits are.
inline void fill_meta(uint8_t *block, const MetaLayout &l, const Distinct &d, bool lookup)
{
    const uint32_t TT = (uint32_t)d.terms.size();
    orr::ScanTerm *st = reinterpret_cast<orr::ScanTerm *>(block + l.terms);
    orr::MatchTerm *mts = reinterpret_cast<orr::MatchTerm *>(block + l.match);
    orr::MatchTerm8 *m8s = reinterpret_cast<orr::MatchTerm8 *>(block + l.match8);
    uint32_t cursor = 0;
    for (uint32_t t = 0; t < TT; ++t) {
        const std::string_view term = d.terms[t];
        st[t].off = cursor;
        st[t].len = (uint32_t)term.size();
        uint32_t pre = 0, msk = 0;
        for (uint32_t k = 0; k < 4 && k < st[t].len; ++k) {
            pre |= (uint32_t)(uint8_t)term[k] << (8 * k);
            msk |= 0xFFu << (8 * k);
        }
        st[t].prefix = pre;
        st[t].mask = msk;
        orr::MatchTerm &mt = mts[t];
        memset(&mt, 0, sizeof(mt));
        mt.len = st[t].len;
        for (uint32_t k = 0; k < 16 && k < st[t].len; ++k) {
            mt.w[k >> 2] |= (uint32_t)(uint8_t)term[k] << (8 * (k & 3));
            mt.m[k >> 2] |= 0xFFu << (8 * (k & 3));
        }
        orr::MatchTerm8 &m8 = m8s[t];
        memset(&m8, 0, sizeof(m8));
        m8.len = st[t].len;
        for (uint32_t k = 0; k < 32 && k < st[t].len; ++k) {
            m8.w[k >> 2] |= (uint32_t)(uint8_t)term[k] << (8 * (k & 3));
            m8.m[k >> 2] |= 0xFFu << (8 * (k & 3));
        }
        if (!term.empty()) memcpy(block + l.pool + cursor, term.data(), term.size());
        cursor += st[t].len;
    }
    if (lookup) {   // the terms of at most 16 bytes sorted by (class = min(bytes, 4), length-masked first dword): vocab_match_lookup
        uint32_t *lk = reinterpret_cast<uint32_t *>(block + l.lk), *keys = lk + kLkHead, *tix = keys + TT;
        std::vector<std::pair<uint64_t, uint32_t>> order;
        order.reserve(TT);
        for (uint32_t t = 0; t < TT; ++t)
            if (st[t].len >= 1 && st[t].len <= 16)
                order.emplace_back(((uint64_t)(std::min<uint32_t>(st[t].len, 4u) - 1u) << 32) | mts[t].w[0], t);
        std::sort(order.begin(), order.end());
        for (int c = 0; c <= 4; ++c) lk[c] = 0;
        for (size_t i = 0; i < order.size(); ++i) {
            keys[i] = (uint32_t)order[i].first;
            tix[i] = order[i].second;
            lk[(order[i].first >> 32) + 1] = (uint32_t)i + 1;
        }
        for (int c = 1; c <= 4; ++c) lk[c] = std::max(lk[c], lk[c - 1]);     // empty classes inherit the boundary in front of them
        lk[5] = lk[6] = lk[7] = 0;
        uint32_t *bloom = reinterpret_cast<uint32_t *>(block + l.bloom);
        memset(bloom, 0, orr::kVocabBloomBits / 8);
        for (const auto &o : order) {
            const uint32_t hb = orr::vocab_bloom_hash((uint32_t)o.first, (uint32_t)(o.first >> 32));
            bloom[hb >> 5] |= 1u << (hb & 31u);
        }
    }
    memcpy(block + l.qmeta, d.qmeta.data(), sizeof(uint32_t) * d.qmeta.size());
    uint32_t *iota = reinterpret_cast<uint32_t *>(block + l.iota);
    for (uint32_t i = 0; i < kIota; ++i) iota[i] = i;
}

// ---- which kernels
// true: the lookup form.  forced: the call's override (-1 none, 0 all-pairs, 1 lookup); env: the environment's, likewise.
// (The lookup pays from tens of millions of (token, term) pairs on: below, sorting the terms on the host -- 0.15 ms for the
// 3,000 terms of 1024 queries -- costs more than comparing them all on the GPU.)
inline bool short_form(uint32_t TT, int64_t n_tokens, int forced, int env)
{
    if (forced >= 0) return forced != 0;
    if (env >= 0) return env != 0;
    return TT >= 64 && (int64_t)TT * n_tokens >= ((int64_t)1 << 25);
}

// Entries at the front of the list of long tokens (n_vlong of them, the first n_vmid of 17 .. 32 bytes) that go one lane per
// token.  forced: the call's override (-1 none, 0 off); env_off: the environment switched the kernel off.
inline int64_t mid_tokens(int64_t n_vmid, int64_t n_vlong, int forced, bool env_off)
{
    return (forced >= 0 ? forced == 0 : env_off) ? 0 : std::min<int64_t>(n_vmid, n_vlong);
}

// ---- the hit list
constexpr uint64_t kHitBytes = 24;      // sizeof(orr::KwHit) (orr_kernels.h asserts it)
constexpr int kMaxRuns = 4;             // runs of a chain, the first included, before "the keyword hit list kept overflowing"

struct HitList {
    uint32_t max_hits;                  // entries reserved
    bool overflow_possible;             // fewer than every (token, term) pair: the count is checked behind the run
};
inline HitList hit_list(int64_t n_tokens, uint32_t TT, uint32_t cap)
{
    const uint64_t want = (uint64_t)std::max<int64_t>(n_tokens, 1) * TT;
    const uint32_t max_hits = (uint32_t)std::min<uint64_t>(want, cap);
    return HitList{max_hits, want > (uint64_t)max_hits};
}

struct AfterRun {
    enum Kind { Stands, Grow, Refused } kind;
    uint32_t new_cap;                   // Grow: the lane's cap from now on
};
inline AfterRun after_run(uint32_t hits, uint32_t max_hits)
{
    if (hits <= max_hits) return AfterRun{AfterRun::Stands, 0u};
    if ((uint64_t)hits * kHitBytes > ((uint64_t)8 << 30)) return AfterRun{AfterRun::Refused, 0u};      // 8 GiB of KwHit
    return AfterRun{AfterRun::Grow, hits + hits / 4 + 1024u};
}

}  // namespace keyword
