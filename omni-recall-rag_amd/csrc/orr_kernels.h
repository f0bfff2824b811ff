// orr_kernels.h -- launch wrappers of the gfx950 kernels behind libomnirecall_hip.so.
// All launches are asynchronous on the given stream; none allocates or synchronises.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/omnirecall_hip.h"
#include "orr_layout.h"
#include "orr_scope_plan.h"
#include "orr_mask_plan.h"
#include "orr_scope_set_plan.h"
#include "orr_scope_terms_plan.h"
#include "orr_scope_near_plan.h"
#include "orr_range_plan.h"
#include "orr_diverse_plan.h"
#include "orr_per_key_plan.h"
#include "orr_key_groups_plan.h"
#include "orr_cluster_key_groups_plan.h"
#include "orr_centroid_index_plan.h"
#include "orr_routed_plan.h"
#include "orr_keyword_plan.h"

#include <atomic>

namespace orr {

// Per-DEVICE launch state (orr_cluster drives several devices from one process, one host thread per shard): the
// max-dynamic-LDS attribute of a kernel and a device's CU count are established on every device they are used on, not on
// whichever device happened to be current at the first call of the process.
inline int current_device_ordinal()
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0) d = 0;
    return d;
}
template <auto KERNEL>
hipError_t ensure_max_dynamic_lds(int bytes)
{
    static std::atomic<uint64_t> done[4] = {};            // one bit per device ordinal (256 devices)
    const int dev = current_device_ordinal() & 255;
    if ((done[dev >> 6].load(std::memory_order_acquire) >> (dev & 63)) & 1ull) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done[dev >> 6].fetch_or(1ull << (dev & 63), std::memory_order_release);
    return e;
}
inline int device_cu_count()
{
    static std::atomic<int> cus[256] = {};
    const int dev = current_device_ordinal() & 255;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = -1;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n > 0 ? n : 0;
}

constexpr int kSelWidth = 64;        // entries a wave keeps while selecting (one per lane)
constexpr int kSelSegRows = 4096;    // rows one workgroup of fuse_select scans
constexpr int kMaxExactQ = 8;        // queries one launch of the exact dot kernel carries
constexpr int kMaxScanTerms = 64;    // query terms one launch of the keyword scan carries
constexpr int kMaxGemvScreenQ = 8;   // queries one launch of the streaming screen (K2g) carries
constexpr int kMaxI8ScreenQ = 4;     // ... of its int8 form (K2i): two accumulators per query and row
constexpr int kCountPlanes = 4;      // 32-bit words per (32 queries, row) of keyword match counts: four bits per query (saturating at 15)

// One selection entry: `key` orders scores (see score_key in the .hip), `pos` is the
// row's position in the shard's candidate order.  key 0 = empty slot.
struct SelEntry {
    unsigned long long key;
    uint32_t pos;
    uint32_t pad;
};

// (ScanTerm, the per-term metadata of the keyword scan: orr_keyword_plan.h)

// K0 / K1e: out[q][r] = sum_i (double)fl32(Q[q][i] * E[r][i]) in index order (exact
// reference arithmetic, RecallSearchService.cs:77-82).  self_norm: Q is ignored and
// out[0][r] = sum_i (double)fl32(E[r][i]^2).  nq <= kMaxExactQ.
hipError_t launch_dot_exact(const float *E, int64_t n_rows, int32_t D, const float *Q, int32_t nq,
                            bool self_norm, double *out, int64_t out_stride, hipStream_t s);

// K3: matches[b][r] = number of terms of query b that occur in row r's content
// (RecallSearchService.cs:111).  n_terms <= kMaxScanTerms; q_term_off[B+1] indexes
// into terms[0..n_terms).  accumulate != 0 adds to matches instead of overwriting (a
// query with more than kMaxScanTerms terms is scanned in several launches).
// Pool layout: row r occupies [cstart[r], cstart[r]+clen[r]), cstart 16-byte aligned,
// followed by 1..16 space bytes; the pool is over-allocated by kScanPoolSlack bytes.
// Terms must not contain whitespace bytes.
// (kScanPoolSlack, kRowAlign, padded_row_bytes: orr_layout.h)
hipError_t launch_keyword_scan(const uint8_t *pool, const uint64_t *cstart, const uint32_t *clen, int64_t n_rows,
                               const uint8_t *term_pool, const ScanTerm *terms, int32_t n_terms,
                               const uint32_t *q_term_off, int32_t B, uint16_t *matches,
                               int64_t matches_stride, int32_t accumulate, hipStream_t s);

// The same scan over the shard's VOCABULARY for every distinct query term at once (one launch).
hipError_t launch_vocab_scan(const uint8_t *vpool, const uint64_t *vstart, const uint32_t *vlen, int64_t n_tokens,
                             const uint8_t *term_pool, const ScanTerm *terms, int32_t n_terms, const uint32_t *identity,
                             uint16_t *vmatch, hipStream_t s);

// Keyword side of a batch as the scoring kernels see it: one row bitmap per DISTINCT
// query term (bit r of bitmaps[t*words_per_term + r/32] = term t occurs in row r) and
// each query's list of distinct-term indices.  bitmaps == nullptr: no query has terms.
struct KwView {
    const uint32_t *bitmaps;
    int64_t words_per_term;
    const uint32_t *q_term_idx;    // [sum of query term counts]
    const uint32_t *q_term_off;    // [B+1]
    // Where distinct term t's bitmap starts, in words from `bitmaps` (null: t * words_per_term).  A term whose only hit is a
    // vocabulary token with a STORED bitmap (orr_index: built once per sealed shard for the frequent tokens) points straight at
    // that bitmap -- the offset then leads out of the batch's own bitmaps into the token store, nothing is expanded or copied.
    const int64_t *term_word_off;
};
__host__ __device__ inline int64_t kw_term_base(const KwView &kw, uint32_t t)
{
    return kw.term_word_off ? kw.term_word_off[t] : (int64_t)t * kw.words_per_term;
}

// One (term, token) match: the token's posting run and where its 1024-posting chunks start.
struct KwHit {
    uint64_t post_begin;
    uint32_t post_len;      // postings of the token (a shard holds fewer than 2^32 rows)
    uint32_t chunk_base;
    uint32_t term;
    uint32_t token;         // vocabulary token of the hit (launch_kw_alias: a term whose ONLY hit is a token with a stored bitmap needs no expansion)
};
static_assert(sizeof(KwHit) == keyword::kHitBytes, "keyword::after_run sizes the hit list");
constexpr uint32_t kPostChunk = 1024;

// token_ids != nullptr: the scanned rows were the vocabulary tokens token_ids[0..n_tokens) (the long ones)
hipError_t launch_vocab_hits(const uint16_t *vmatch, int64_t n_tokens, int32_t n_terms, const uint32_t *token_ids,
                             const uint64_t *post_off, unsigned long long *counter, KwHit *hits, uint32_t max_hits, hipStream_t s);

// (MatchTerm, MatchTerm8 -- a query term for the lane-per-token matchers -- kVocabBloomBits and vocab_bloom_hash: orr_keyword_plan.h)
constexpr int kMatchGroup = 32;       // terms per workgroup (grid.y)
// Every token of at most 16 bytes against every term, hits reserved as by launch_vocab_hits.
hipError_t launch_vocab_match_short(const uint8_t *vpool, const uint64_t *vstart, const uint32_t *vlen, int64_t n_tokens,
                                    const MatchTerm *terms, int32_t n_terms, const uint64_t *post_off,
                                    unsigned long long *counter, KwHit *hits, uint32_t max_hits, hipStream_t s);
// Tokens of at most 16 bytes against MANY terms: the terms (of at most 16 bytes) sorted by their length-masked first dword in
// four classes (lk[0..4] = class boundaries in keys / tidx; 1, 2, 3, 4+ bytes), every window of a token looked up.
// bloom: kVocabBloomBits bits, bit vocab_bloom_hash(key, class) set for every (class, key) of the tables.
hipError_t launch_vocab_match_lookup(const uint8_t *vpool, const uint64_t *vstart, const uint32_t *vlen, int64_t n_tokens,
                                     const MatchTerm *terms, const uint32_t *lk, const uint32_t *keys, const uint32_t *tidx,
                                     const uint32_t *bloom, const uint64_t *post_off, unsigned long long *counter, KwHit *hits,
                                     uint32_t max_hits, hipStream_t s);
// The tokens of 17..32 bytes of a list (start, length, token number) against every term (longer terms cannot occur in them),
// one lane per token.
hipError_t launch_vocab_match_mid(const uint8_t *vpool, const uint64_t *starts, const uint32_t *lens, const uint32_t *ids, int64_t n_list,
                                  const MatchTerm8 *terms, int32_t n_terms, const uint64_t *post_off, unsigned long long *counter,
                                  KwHit *hits, uint32_t max_hits, hipStream_t s);
// counter_host (optional, pinned host memory): receives *counter (hits << 32 | chunks) for the caller's statistics.
// skip_term (optional, [terms]): hits of terms flagged there are left out (their bitmaps are aliases, launch_kw_alias).
hipError_t launch_expand_hits(const KwHit *hits, const unsigned long long *counter, uint32_t max_hits,
                              const uint32_t *post_rows, uint32_t *bitmaps, int64_t words_per_term, hipStream_t s,
                              unsigned long long *counter_host = nullptr, const uint8_t *skip_term = nullptr);
// Decides per distinct term of a batch whether its bitmap can be an ALIAS of a stored token bitmap: exactly one (term, token)
// hit, and that token has a stored bitmap (tok_bm_index[token] >= 0: bitmap number in a store that begins bm_store_delta
// words from the batch's bitmaps).  term_cnt [n_terms] must be zero on entry.  Out: term_word_off [n_terms], alias [n_terms].
hipError_t launch_kw_alias(const KwHit *hits, const unsigned long long *counter, uint32_t max_hits, int32_t n_terms,
                           const int32_t *tok_bm_index, int64_t bm_store_delta, int64_t words_per_term, uint32_t *term_cnt,
                           uint32_t *term_tok, int64_t *term_word_off, uint8_t *alias, hipStream_t s);

// Per-query constants of the fused score.
struct QueryConst {
    double norm_a;        // exact sum_i (double)fl32(q_i^2); unused when use_cos == 0
    double inv_sqrt_na;   // 1/sqrt(norm_a) for the batched selection score
    double inv_n_terms;   // 1/queryTerms.Length, 0 without terms
    int32_t n_terms;      // queryTerms.Length (RecallSearchService.cs:112)
    int32_t use_cos;      // query dim == index dim, dim > 0 (and norm_a > 0 in the batched form); | kQueryKeepAll
};

// Bit of QueryConst::use_cos (which every reader but the two below takes as a truth value): the query's products with the rows
// are subnormal in fp32 (0 < norm_a < D 2^-96, which holds whenever 0 < max|q| < 2^-48), where the relative product error the
// float forms charge does not hold.  Set for queries in device memory, which plan_form cannot look at, where the pass has no
// int8 per-pair bound: fuse_select and the bf16 streaming screen keep every pair of such a query (a floor takes nothing from
// them), so the query comes back uncertified and climbs the ladder to the exact pass.  No host synchronisation in front of the pass.
constexpr int32_t kQueryKeepAll = 2;

// qc[b].norm_a / inv_sqrt_na / use_cos from norms computed on the device (launch_dot_exact, self_norm over the queries).
hipError_t launch_patch_query_norms(QueryConst *qc, const double *norm_a, int32_t B, bool batched, hipStream_t s,
                                    double *norm_host = nullptr,         // norm_host (optional, pinned): the norms for the host as well
                                    const QueryConst *qc_host = nullptr,   // qc_host (optional, pinned): the constants come from there, not from qc
                                    double tiny_below = 0.0);              // > 0: norms in (0, tiny_below) set kQueryKeepAll

// Per-row selection constants for a batch: out[r] = {1/sqrt(normB) or 0, recency * 0.1}.
hipError_t launch_row_consts(const double *norm_b, const int64_t *created, int64_t now_ticks, int64_t n_rows,
                             double2 *out, hipStream_t s);

// K4+K5a: fused score per (query,row) and per-workgroup top-64.
//   score = (cos*0.7) + (kw*0.2) + (rec*0.1)  in fp64, left to right (…cs:66)
// out_sel: [B][n_seg][kSelWidth] entries, best first.  n_seg = ceil(n_rows / kSelSegRows).
// dot (fp64, exact pass) or dotf (fp32, K2 candidate pass): exactly one is non-null when cosine applies.
// row_consts != nullptr selects the batched (reciprocal-multiply) form of the score.
// Scans segments [seg_first, seg_first+seg_count); tau != nullptr: per-query key a row must
// exceed to be considered (the k'-th best key of an already scanned prefix).
// i8.rowf != nullptr (with row_consts): dotf holds the INTEGER dots of the int8 screening GEMM over these rows
// (launch_screen_i8_dots); the key is then a LOWER bound of the score: score(dot^) minus the per-pair bound.
struct I8Prefix {
    const float4 *rowf = nullptr;    // launch_i8_rowf
    const float *qs1 = nullptr;      // [B] query scales
    const double *qerr2 = nullptr;   // [B] |q - q^|^2 of the one-level queries
};
hipError_t launch_fuse_select(const double *dot, const float *dotf, int64_t dot_stride, const double *norm_b,
                              const int64_t *created, const double2 *row_consts, KwView kw,
                              const QueryConst *qc, int64_t now_ticks, int64_t n_rows, int32_t B,
                              int32_t seg_first, int32_t seg_count, const unsigned long long *tau,
                              SelEntry *out_sel, int32_t n_seg_stride, hipStream_t s, I8Prefix i8 = I8Prefix(),
                              int floor_only = 0);          // floor_only 1: lists of per-lane maxima (enough for a floor key; FAST rows, no tau);
                                                            // 2: 16 wave maxima per list, nothing sorted (launch_select_final_sample wave_maxima = 1)

// K5b: merges the per-workgroup lists of each query and writes kprime candidate
// records plus the trailer ([B][kprime+1], see orr_candidate).
// tau_out != nullptr: write only the k'-th best key per query (sampling pass), no records.
// approx_eps goes into the trailer's `dot` field: the bound on |selection score - exact score|
// of the pass that produced the records (0 for the exact pass).
hipError_t launch_select_final(const SelEntry *sel, int32_t n_seg, int32_t B, int32_t kprime,
                               int64_t n_rows, int64_t row_base, const double *dot, const float *dotf,
                               int64_t dot_stride, const double *norm_b, const int64_t *created,
                               const int64_t *row_ids, KwView kw, int32_t dot_exact, double approx_eps,
                               unsigned long long *tau_out, const uint32_t *fused_cnt, uint32_t fused_cap,
                               const double *two_stage_L, orr_candidate *out, hipStream_t s);

// Fused epilogue of the batched candidate pass: score, compare with the query's floor key,
// append survivors to the query's buffer (cap entries; cnt keeps counting past it).
struct FusedEpilogue {
    const double2 *rowc;               // per-row {1/sqrt(normB) or 0, recency*0.1}
    const QueryConst *qc;
    KwView kw;
    const unsigned long long *tau;     // [B] floor keys
    const float4 *qf;                  // [B] fp32 pre-filter constants (launch_fused_query_consts)
    const uint32_t *count_planes;      // [kCountPlanes][ceil(B/32)][plane_stride] match counts, word k = queries 8k..8k+7 of the group, 4 bits each; or null
    int64_t plane_stride;
    // int8 screening GEMM (K2j) only, else null: per row {se_r, 0.7 (rel_err + 2^-22), rel_hat, 0}; per query s1.
    // The accumulator then holds the integer dot I: dot^ = s1 se_r I, and qf.x / qf.w carry s1 0.7/sqrt(normA)
    // and 0.7 |q - q^| / sqrt(normA): score bound = score(dot^) + rowf.y + qf.w rowf.z.
    const float4 *i8_rowf;
    const float *i8_qs1;
    uint32_t *cnt;                     // [B]
    SelEntry *buf;                     // [B][cap]
    uint32_t cap;
    unsigned long long *stamps;        // diagnostic (ORR_SCREEN_STAMPS=file): s_memtime at the phases of every output tile, else null
    int32_t count_bits;                // 4 (or 0: the same): count words as described above; 2: TWO bits per (query,row) -- word kk = queries 16 kk .. 16 kk + 15 of the group, two words per (32 queries, row) -- for batches whose queries all have at most three terms (the 16 x 16 x 64 form only)
    const float4 *qf16;                // [B] the 16 x 16 x 64 form's staged constants: qf with everything finite and .w = the batch's largest query bound term (launch_fused_query_consts)
    uint32_t *tickets;                 // [8] zeroed counters of ONE launch of the 16 x 16 x 64 screening GEMM (output tiles beyond a workgroup's first two are drawn from them), or null: static assignment
};
// K2b: S (or the fused epilogue) from three bf16 MFMA products of hi/lo splits (see orr_gemm.hip
// for the error bound); D % 64 == 0.  q_split_ws: 4*B*D bytes filled by launch_split_queries.
hipError_t launch_split_queries(const float *Q, int32_t B, int32_t D, void *q_split_ws, hipStream_t s);
hipError_t launch_gemm_dot_bf16x3(const void *q_split_ws, int32_t B, const float *E, int64_t row_first, int64_t n_rows, int32_t D,
                                  float *S, int64_t s_stride, const FusedEpilogue *epi, int32_t products, hipStream_t s);
// rows [row_first, row_end) only (row_first % 256 == 0; row_end < 0: to the end)
// bits = 2: two-bit counts (every query of the batch has at most three terms), half the words (see FusedEpilogue::count_bits)
hipError_t launch_query_count_planes(KwView kw, int32_t B, int64_t n_rows, int64_t plane_stride, uint32_t *planes, hipStream_t s,
                                     int64_t row_first = 0, int64_t row_end = -1, int32_t bits = 4);
// whether launch_screen_i8 runs its 16 x 16 x 64 form for this shape (the only form that reads two-bit count words)
bool screen_i8_uses_tile16(int32_t B, int64_t n_rows, int32_t D, int64_t plane_stride);
// which form of the tile launch_screen_i8 runs for this shape and epilogue: 0 eight-wave, 1 four-wave 32 x 32 x 32, 2 four-wave
// 16 x 16 x 64 (orr_index_screen_i8_dots numbers them the same way)
int32_t screen_i8_form(int32_t B, int64_t n_rows, int32_t D, const FusedEpilogue &epi);
// qf16 (optional, [B]): the same constants made safe for a NaN-dropping test (fused_epilogue16) -- finite qx / qz, a query with
// anything non-finite turned into "every pair passes" (qx = qz = 0, floor -inf) -- with .w = the largest finite query bound
// term of the batch in EVERY entry.
// zero_a / zero_b (optional): words this launch clears as well (the pass's counters, the screening launches' tickets).
hipError_t launch_fused_query_consts(const QueryConst *qc, const unsigned long long *tau, int32_t B, float4 *qf, hipStream_t s,
                                     const float *i8_qs1 = nullptr, const double *i8_qerr2 = nullptr, float4 *qf16 = nullptr,
                                     uint32_t *zero_a = nullptr, int32_t n_a = 0, uint32_t *zero_b = nullptr, int32_t n_b = 0);
// K2c (orr_screen.hip): plain-bf16 screening GEMM (256 x 256 x 64 tiles, LDS-DMA staging) over TILED bf16
// images of the embeddings (the shard's shadow) and of the batch's queries; S or the fused epilogue as above.
size_t bf16_tiled_bytes(int64_t n_rows, int32_t D);
hipError_t launch_bf16_tiled(const float *X, int64_t n_rows, int32_t D, void *out, hipStream_t s);
hipError_t launch_screen_bf16(const void *q_tiled, int32_t B, const void *e_shadow, int64_t row_first, int64_t n_rows,
                              int32_t D, float *S, int64_t s_stride, const FusedEpilogue *epi, hipStream_t s);
// K2g: the screening pass for 1..kMaxGemvScreenQ queries as a stream over the tiled shadow (no matrix core).
hipError_t launch_screen_gemv_bf16(const void *q_hi, int32_t B, const void *e_shadow, int64_t n_rows, int32_t D,
                                   const FusedEpilogue &epi, hipStream_t s);
// K2i: the streaming screen over an INT8 shadow (per-row scale, two-level int8 queries, exact integer dots,
// a per-pair Cauchy-Schwarz bound from the quantisation norms) -- see orr_screen.hip.  D % 128 == 0.
size_t i8_tiled_bytes(int64_t n_rows, int32_t D);
hipError_t launch_i8_shadow(const float *E, const double *norm_b, int64_t n_rows, int32_t D, void *tiled, float *scale,
                            float *rel_err, float *rel_hat, hipStream_t s);
// orr_index_update_rows: targets t = 0..n_targets-1 get staged row src[t] - src_base of `rows` ([.][D] fp32, compact) and its
// exact norm (norms[], launch_dot_exact self_norm over `rows`) at position pos[t] of E / norm_b, and, where the shadows exist
// (non-null), the int8 image + scale / rel_err / rel_hat / rowf (D % 128 == 0) and the tiled bf16 image (D % 64 == 0) that
// launch_i8_shadow + launch_i8_rowf and launch_bf16_tiled would write there.  Targets must be distinct positions.
hipError_t launch_update_rows(const float *rows, const double *norms, const int64_t *pos, const int64_t *src, int64_t src_base,
                              int64_t n_targets, int32_t D, float *E, double *norm_b, void *i8_tiled, float *i8_scale, float *i8_rel_err,
                              float *i8_rel_hat, float4 *i8_rowf, void *bf16_tiled, hipStream_t s);
// zero (optional): n_zero words the kernel clears as well (the pass's counters: saves the call a memset).
hipError_t launch_i8_queries(const float *Q, int32_t B, int32_t D, void *q12, float *s1, double *err2, hipStream_t s,
                             double *err2_level1 = nullptr, uint32_t *zero = nullptr, int32_t n_zero = 0);
// norm_b / created / now_ticks: not null -> the kernel forms each row's scoring constants itself (epi.rowc unused).
// lower_bound with screen_gemv_i8_prefix_makes_lists(D): epi.tau must be all 0 and the keys leave as sorted lists of 64
// in epi.buf[b][0 .. ceil(n_rows / 64) * 64) (epi.cnt unused); otherwise survivors are appended to epi.buf through epi.cnt.
bool screen_gemv_i8_prefix_makes_lists(int32_t D);
hipError_t launch_screen_gemv_i8(const void *q12, const float *s1, const double *err2, int32_t B, const void *tiled,
                                 const float *scale, const float *rel_err, const float *rel_hat, const double *norm_b,
                                 const int64_t *created, int64_t now_ticks, int64_t n_rows, int32_t D,
                                 const FusedEpilogue &epi, bool lower_bound, hipStream_t s);
// Diagnostic: the raw accumulators of the same kernel, S[b][0][r] = I1 and S[b][1][r] = I2 for 1..kMaxI8ScreenQ queries, in the
// 16-row-unit form of the sampled prefix (fine; D % 1024 == 0) or the 128-row-unit form of the pass over all rows.
hipError_t launch_screen_gemv_i8_dots(const void *q12, int32_t B, const void *tiled, int64_t n_rows, int32_t D, int32_t *S, bool fine,
                                      hipStream_t s);
// K2j: the screening GEMM on the int8 shadow (v_mfma_i32_32x32x32_i8: twice the bf16 rate, half its bytes).
// Queries: ONE int8 level (q1 of launch_i8_queries, err2_l1), tiled like the rows; epi must carry i8_rowf / i8_qs1.
hipError_t launch_i8_rowf(const float *scale, const float *rel_err, const float *rel_hat, int64_t n_rows, float4 *rowf, hipStream_t s);
hipError_t launch_i8_tile_queries(const void *q1_linear, int32_t B, int32_t D, void *tiled, hipStream_t s);
// rows [row_first, n_rows) (row_first % 256 == 0): a launch per row range lets the count words of later ranges be formed
// while earlier ranges are multiplied
hipError_t launch_screen_i8(const void *q_tiled, int32_t B, const void *e_tiled, int64_t n_rows, int32_t D,
                            const FusedEpilogue &epi, hipStream_t s, int64_t row_first = 0);
// The same product over rows [0, n_rows) with the integer dots written out: S[b][r] = (float)I (the sampled prefix).
hipError_t launch_screen_i8_dots(const void *q_tiled, int32_t B, const void *e_tiled, int64_t n_rows, int32_t D, float *S,
                                 int64_t s_stride, hipStream_t s);
// Diagnostic: the raw int32 accumulators of one FORM of the kernel (0 eight-wave, 1 four-wave 32 x 32 x 32, 2 four-wave
// 16 x 16 x 64; forms 1 and 2 need D / 64 > 6), rows requested non-temporal or not; and the shadow untiled again.
hipError_t launch_screen_i8_dots_raw(const void *q_tiled, int32_t B, const void *e_tiled, int64_t n_rows, int32_t D, int32_t *S,
                                     int64_t s_stride, int32_t form, bool nt_rows, hipStream_t s, uint32_t *tickets = nullptr);
hipError_t launch_i8_untile(const void *tiled, int64_t n_rows, int32_t D, void *out_linear, hipStream_t s);
// Two-stage pass helpers (orr_gemm.hip).
hipError_t launch_rescore_buffer_exact(const float *E, int32_t D, const float *Q, int32_t B, const double *norm_b,
                                       const int64_t *created, KwView kw, const QueryConst *qc, int64_t now_ticks,
                                       const uint32_t *cnt, uint32_t cap, SelEntry *buf, double *buf_dot, hipStream_t s);
// Up to 256 queries (the caller's choice), D % 256 == 0: re-score + lists + final selection + records with exact dots in one launch (done: [B]
// zeroed counters; recs / cnt_host may be pinned host memory).
hipError_t launch_finish_survivors(const float *E, int32_t D, const float *Q, int32_t B, const double *norm_b, const int64_t *created,
                                   const int64_t *row_ids, KwView kw, const QueryConst *qc, int64_t now_ticks, const uint32_t *cnt,
                                   uint32_t *done, uint32_t cap, SelEntry *buf, double *buf_dot, SelEntry *lists, int32_t kprime,
                                   int64_t n_rows, int64_t row_base, const double *two_stage_L, orr_candidate *recs, uint32_t *cnt_host,
                                   hipStream_t s);
// survivors per group of that launch (its `lists`: B x cap / group x kSelWidth entries); 0 = groups of 64
int32_t finish_survivors_group(int32_t B, int32_t D);
hipError_t launch_records_dot_from_buffer(const SelEntry *buf, const double *buf_dot, const uint32_t *cnt, uint32_t cap, int32_t B,
                                          int32_t kprime, int64_t row_base, orr_candidate *recs, hipStream_t s);
hipError_t launch_buffer_to_lists(const SelEntry *buf, const uint32_t *cnt, uint32_t cap, int32_t B, int32_t seg_first,
                                  int32_t n_seg_total, SelEntry *out_sel, hipStream_t s);
// K2s: the same for B <= 32 queries, streaming (HBM-bound) structure.
hipError_t launch_gemv_mfma(const float *Q, int32_t B, const float *E, int64_t n_rows, int32_t D, float *S,
                            int64_t s_stride, hipStream_t s);
// K6: recomputes records[b][c].dot in the reference's exact arithmetic for every valid record
// (row = order_key - row_base) and sets ORR_CAND_DOT_EXACT.
hipError_t launch_rescore_exact(const float *E, int32_t D, const float *Q, int32_t B, int32_t kprime, int64_t row_base,
                                orr_candidate *recs, hipStream_t s);

// Sampling pass of the batched selection: tau_out[b] = k'-th best key among the first sample_seg
// lists of query b (0 if there are fewer).
// floor (optional): the two-stage floor of that key in the same launch (floor_key[b], L[b]; two_stage_floor_of, orr_device.h).
struct FloorOut {
    unsigned long long *floor_key = nullptr;
    double *L = nullptr;
    double eps3 = 0.0, eps1 = 0.0;
};
hipError_t launch_select_final_sample(const SelEntry *sel, int32_t n_seg_total, int32_t sample_seg, int32_t B,
                                      int32_t kprime, unsigned long long *tau_out, hipStream_t s, FloorOut floor = FloorOut(),
                                      int32_t wave_maxima = 0,     // 1: the lists hold 16 unsorted wave maxima each (fuse_select floor_only = 2)
                                      int32_t merge_all = 0);      // 1: never from the lists' heads alone (some query's lists may be empty: a grouped pass)

// Generic path for large k: keys[r] = score key of (query b,row r), vals[r] = r.
hipError_t launch_score_keys(const double *dot, const double *norm_b, const int64_t *created,
                             KwView kw, int32_t b, QueryConst qc, int64_t now_ticks, int64_t n_rows,
                             unsigned long long *keys, uint32_t *vals, hipStream_t s);
// Device radix sort (descending, stable) of (keys, vals); temp sizing by query.
hipError_t sort_pairs_desc(void *temp, size_t &temp_bytes, const unsigned long long *keys_in,
                           unsigned long long *keys_out, const uint32_t *vals_in, uint32_t *vals_out,
                           int64_t n, hipStream_t s);
// Builds candidate records for the first K sorted entries (+ trailer at index K).
hipError_t launch_records_from_sorted(const unsigned long long *keys, const uint32_t *vals, int32_t K,
                                      int64_t n_rows, int64_t row_base, const double *dot, int64_t dot_stride,
                                      const double *norm_b, const int64_t *created, const int64_t *row_ids,
                                      KwView kw, int32_t b, int32_t dot_exact, orr_candidate *out,
                                      hipStream_t s);

// Seal-time row permutation (dst[p] = src[perm[p]]).
hipError_t launch_gather_rows_f32(const float *src, float *dst, const int64_t *perm, int64_t n, int32_t D,
                                  hipStream_t s);
hipError_t launch_gather_i64(const int64_t *src, int64_t *dst, const int64_t *perm, int64_t n, hipStream_t s);
// orr_index_insert_rows, the two-source merge: dst row r (r = 0..n-1) <- E row src_idx[r] when src_idx[r] >= 0, else row
// ~src_idx[r] - stage_base of `stage` ([.][D] fp32, the new rows of this round).  16-byte vectors when D % 4 == 0.  dst may
// point into E when no source row of the launch lies inside [dst, dst + n rows).
hipError_t launch_merge_rows_f32(const float *E, const float *stage, const int64_t *src_idx, int64_t stage_base, float *dst,
                                 int64_t n, int32_t D, hipStream_t s);
// ... and one 8-byte value per row: dst[r] = src_idx[r] >= 0 ? old[src_idx[r]] : add[~src_idx[r]] (dst a separate array).
hipError_t launch_merge_i64(const int64_t *old, const int64_t *add, const int64_t *src_idx, int64_t *dst, int64_t n, hipStream_t s);
// Content rows: dst row r <- src row perm[r] (perm == nullptr: identity).
hipError_t launch_gather_content(const uint8_t *src_pool, const uint64_t *src_start, const uint32_t *src_len,
                                 uint8_t *dst_pool, const uint64_t *dst_start, const int64_t *perm, int64_t n,
                                 hipStream_t s);
hipError_t launch_gather_u32(const uint32_t *src, uint32_t *dst, const int64_t *perm, int64_t n, hipStream_t s);
hipError_t launch_iota_i64(int64_t *dst, int64_t n, int64_t base, hipStream_t s);
// Deleted rows: overwrite norm and timestamp at the given positions; flag the records of deleted positions.
hipError_t launch_tombstone_rows(const int64_t *pos, int32_t n, double *norm_b, int64_t *created, hipStream_t s);
hipError_t launch_mark_dead_records(orr_candidate *recs, int32_t B, int32_t kprime, const int64_t *dead, int32_t n_dead,
                                    int64_t row_base, hipStream_t s);


// ---- scoped search (orr_search_batch_scoped; the rules are orr_scope_plan.h's) ----------------------------------------------
// The id table of a sealed shard: ids_out ascending with pos_out the rows' positions (ascending within equal ids), through a
// stable radix sort of (ids_in, 0 .. n-1); pos_in is scratch of n words.  temp == nullptr: only temp_bytes is set.
hipError_t scope_sort_id_table(void *temp, size_t &temp_bytes, const int64_t *ids_in, int64_t *ids_out, uint32_t *pos_in,
                               uint32_t *pos_out, int64_t n, hipStream_t s);
// Listed ids -> bits: bit p of bitmaps[b * words ..) for every live row p (not in dead[], ascending) that carries an id of
// query b's list ids[scope_off[b] .. scope_off[b + 1]) (scope_off == nullptr: one bitmap for the whole list).  The bitmaps
// must be zero on entry; words % 4 == 0, words * 32 >= n_rows.
hipError_t launch_scope_lookup(const int64_t *table_ids, const uint32_t *table_pos, int64_t n_rows, const int64_t *ids, int64_t n_ids,
                               const uint64_t *scope_off, int32_t n_q, const int64_t *dead, int32_t n_dead, uint32_t *bitmaps,
                               int64_t words, hipStream_t s);
constexpr int kScopeChunkWords = 1024;     // words of a bitmap one workgroup counts / compacts (32,768 rows)
inline int32_t scope_chunks(int64_t words) { return (int32_t)((words + kScopeChunkWords - 1) / kScopeChunkWords); }
// chunk_cnt[n_bitmaps][scope_chunks(words)] = set bits per chunk; live[q] = set bits of query q's bitmap, took[q] =
// min(live[q], max(0, limit[q])) (live / took may be pinned host memory).  n_bitmaps is n_q, or 1: all queries share it.
hipError_t launch_scope_counts(const uint32_t *bitmaps, int64_t words, int32_t n_bitmaps, int32_t n_q, const int64_t *limit,
                               uint32_t *chunk_cnt, uint32_t *live, uint32_t *took, hipStream_t s);
// buf[i][0 .. took[qsel[i]]) = the first limit[qsel[i]] set bits of query qsel[i]'s bitmap as entries in candidate order
// (key 1, pos = the row); cap entries per query, nothing is written beyond them.
hipError_t launch_scope_compact(const uint32_t *bitmaps, int64_t words, int32_t n_bitmaps, const uint32_t *chunk_cnt, const uint32_t *qsel,
                                int32_t n_sel, const int64_t *limit, SelEntry *buf, uint32_t cap, hipStream_t s);
// launch_rescore_buffer_exact for any D and for queries without a cosine part (qc.use_cos == 0: Q is not read); also leaves
// the pair's keyword matches in the entry's pad.
hipError_t launch_scope_rescore_generic(const float *E, int32_t D, const float *Q, int32_t B, const double *norm_b, const int64_t *created,
                                        KwView kw, const QueryConst *qc, int64_t now_ticks, const uint32_t *cnt, uint32_t cap, SelEntry *buf,
                                        double *buf_dot, hipStream_t s);
// Every buffered pair of a query as a record (exact dot from buf_dot, ORR_CAND_DOT_EXACT), kprime >= every count; trailer:
// approx_score -inf, order_key = the query's count.
hipError_t launch_scope_records(const SelEntry *buf, const double *buf_dot, const uint32_t *cnt, uint32_t cap, int32_t B, int32_t kprime,
                                int64_t row_base, const double *norm_b, const int64_t *created, const int64_t *row_ids, KwView kw,
                                orr_candidate *recs, hipStream_t s);
// The trailers the two-stage tail wrote, made a scoped pass's: order_key = cnt[b], no floor (ORR_CAND_TWO_STAGE cleared).
hipError_t launch_scope_trailers(orr_candidate *recs, int32_t B, int32_t kprime, const uint32_t *cnt, hipStream_t s);

// ---- masked search (orr_search_batch_masked; the rules are orr_mask_plan.h's) ----------------------------------------------
// *n_clip (may be pinned host memory) = one past the position of the took-th set bit of the bitmap (1 <= took <= its set
// bits; chunk_cnt as launch_scope_counts left it).
hipError_t launch_mask_clip(const uint32_t *bitmap, int64_t words, const uint32_t *chunk_cnt, uint32_t took, int64_t *n_clip, hipStream_t s);
// launch_mask_clip with took = the set bits, for n_slots bitmaps [n_slots][words] with chunk counts [n_slots][scope_chunks(words)] in
// one launch: n_clip[s] (may be pinned host memory) = one past the last set bit of bitmap s, 0 for an empty one.  live [n_slots]: the
// bitmaps' set bits, DEVICE memory (launch_scope_counts wrote them on the same stream).
hipError_t launch_mask_clip_slots(const uint32_t *bitmaps, int64_t words, const uint32_t *chunk_cnt, const uint32_t *live, int32_t n_slots,
                                  int64_t *n_clip, hipStream_t s);
// The front of a grouped pass over scope handles in one launch.  Entry e of the table (e < n_entries <= kMaxGatherGroups): the
// bitmap (`words` words, words % 4 == 0, 16-byte aligned) and chunk counts of a handle are copied to dst_bm[slot[e]][words] and
// dst_chunks[slot[e]][scope_chunks(words)] (slot[e] < n_slots; distinct entries name distinct slots), and where clip_took[e] > 0
// n_clip[slot[e]] (may be pinned host memory) = what launch_mask_clip gives for that bitmap and took, read from the source.
// The table travels by value.  hipErrorInvalidValue before the launch for a bad shape, a null or a misaligned base.
constexpr int32_t kMaxGatherGroups = 64;
constexpr int64_t kGatherMaxBlocksX = 256;
struct GroupGatherTable {
    const uint32_t *bm[kMaxGatherGroups];
    const uint32_t *chunks[kMaxGatherGroups];
    uint32_t clip_took[kMaxGatherGroups];
    int32_t slot[kMaxGatherGroups];
};
hipError_t launch_group_gather_clip(const GroupGatherTable &tab, int32_t n_entries, int32_t n_slots, int64_t words, uint32_t *dst_bm,
                                    uint32_t *dst_chunks, int64_t *n_clip, hipStream_t s);
// launch_row_consts for the rows whose bit is set; {0, mask::kMaskedRecency} for the others.  The bitmap covers n_rows.
hipError_t launch_row_consts_masked(const double *norm_b, const int64_t *created, int64_t now_ticks, int64_t n_rows, const uint32_t *bitmap,
                                    double2 *out, hipStream_t s);
// Per query: buf[b][0 .. min(cnt[b], cap)) compacted in place to the entries mask::survivor_in_scope keeps; cnt[b] = their
// number, or unchanged where cnt[b] > cap (the overflow signal stays).
hipError_t launch_mask_survivors(const uint32_t *bitmap, int64_t n_clip, uint32_t *cnt, uint32_t cap, SelEntry *buf, int32_t B, hipStream_t s);
// out (words, all written) = the set bits of bitmap with rank in [first, last) among its set bits.
hipError_t launch_mask_part(const uint32_t *bitmap, int64_t words, const uint32_t *chunk_cnt, uint64_t first, uint64_t last, uint32_t *out,
                            hipStream_t s);
// The two-stage tail's trailers behind a masked screen: order_key = took, floor and flags kept.
hipError_t launch_mask_trailers(orr_candidate *recs, int32_t B, int32_t kprime, int64_t took, hipStream_t s);

// ---- grouped masked search (orr_search_batch_masked_groups; the rules are orr_group_plan.h's) -------------------------------
// bitmaps[n_groups][words] as launch_scope_lookup leaves them; clip[n_groups] (device): the rows [0, clip[g]) of group g take
// part, 0 for a group that takes no part in the pass.
// launch_row_consts for the rows some group holds in front of its own clip; {0, mask::kMaskedRecency} for the others.
hipError_t launch_row_consts_grouped(const double *norm_b, const int64_t *created, int64_t now_ticks, int64_t n_rows, const uint32_t *bitmaps,
                                     int64_t words, int32_t n_groups, const int64_t *clip, double2 *out, hipStream_t s);
// launch_mask_survivors with the bitmap and the clip of query b's own group, qgroup[b] (device, < n_groups).
hipError_t launch_mask_survivors_grouped(const uint32_t *bitmaps, int64_t words, int32_t n_groups, const int64_t *clip, const uint32_t *qgroup,
                                         uint32_t *cnt, uint32_t cap, SelEntry *buf, int32_t B, hipStream_t s);
// launch_mask_trailers with took[b] (device) per query.
hipError_t launch_mask_trailers_grouped(orr_candidate *recs, int32_t B, int32_t kprime, const int64_t *took, hipStream_t s);

// ---- scope handles (orr_scope; the rules are orr_scope_set_plan.h's) ---------------------------------------------------------
// bitmap (words, all written) = the bits [p0, p1); 0 <= p0, p1 <= words * 32.
hipError_t launch_scope_fill_range(uint32_t *bitmap, int64_t words, int64_t p0, int64_t p1, hipStream_t s);
// The bit of each of pos[0 .. n) (device) cleared.
hipError_t launch_scope_clear_positions(uint32_t *bitmap, int64_t words, const int64_t *pos, int64_t n, hipStream_t s);
// dst = dst AND / OR / ANDNOT src (scope_set::Op), in place; both of `words` words.
hipError_t launch_scope_combine(uint32_t *dst, const uint32_t *src, int64_t words, int32_t op, hipStream_t s);
// new_bm[g] (new_words words, all written) = old_bm[g] carried through a move of rows, for n_scopes bitmaps at once (the pointer
// arrays are device memory): destination row d < first keeps its bit, row first + r < n_new takes the bit of old position
// src[r] (device, n_new - first entries), none when src[r] < 0.  new_bm[g] must not alias old_bm[g].
hipError_t launch_scope_remap(const int64_t *src, int64_t first, int64_t n_new, int64_t new_words, const uint32_t *const *old_bm,
                              int64_t old_words, uint32_t *const *new_bm, int32_t n_scopes, hipStream_t s);
// out[i] = row_ids[buf[i].pos] for the n entries launch_scope_compact left.
hipError_t launch_scope_entry_ids(const SelEntry *buf, int64_t n, const int64_t *row_ids, int64_t n_rows, int64_t *out, hipStream_t s);

// ---- row keys and the per-key search (orr_keys, orr_search_batch_per_key; the rules are orr_per_key_plan.h's) -----------------
// out[s][words] for s < n_slots (all words written) = base AND NOT the rows whose key slot s has closed: key [n_rows] the key
// column, tab_keys / tab_masks [n_tab] the sorted union table (per_key::build_table; LDS up to per_key::kLdsTable entries, global
// memory beyond).  base: words % 4 == 0, 16-byte aligned, bits at or above n_rows clear; out 16-byte aligned.  No atomics.
hipError_t launch_keys_exclude(const int64_t *key, int64_t n_rows, const uint32_t *base, int64_t words, const int64_t *tab_keys,
                               const uint64_t *tab_masks, int32_t n_tab, int32_t n_slots, uint32_t *out, hipStream_t s);
// The opposite rule (orr_search_batch_routed; orr_routed_plan.h): out[s][words] for s < n_slots (all words written) = base AND the
// rows whose key slot s routed to.  The arguments and what is refused are launch_keys_exclude's; base is read only by the
// workgroups that hold a routed row.
hipError_t launch_keys_include(const int64_t *key, int64_t n_rows, const uint32_t *base, int64_t words, const int64_t *tab_keys,
                               const uint64_t *tab_masks, int32_t n_tab, int32_t n_slots, uint32_t *out, hipStream_t s);
// The bit of position pos[i] cleared in bitmap slot[i] of bitmaps[.][words], for n (slot, position) pairs (device).
hipError_t launch_keys_clear_seen(uint32_t *bitmaps, int64_t words, int32_t n_slots, const int32_t *slot, const int64_t *pos, int64_t n,
                                  hipStream_t s);
// bm (words, all written) = bit r set iff row r < n_rows carries a key of tab_keys [n_tab] (ascending, distinct; ORR_KEY_NONE may
// be listed and then selects the rows without a key).  words % 4 == 0.
hipError_t launch_keys_member(const int64_t *key, int64_t n_rows, const int64_t *tab_keys, int32_t n_tab, uint32_t *bm, int64_t words,
                              hipStream_t s);
// out[i] = key[pos[i]] (ORR_KEY_NONE for a position outside the shard).  With the id table (table_ids non-null) pos[i] is a
// row id: the key of the first live row that carries it, ORR_KEY_NONE when there is none.
hipError_t launch_keys_gather(const int64_t *key, int64_t n_rows, const int64_t *pos, int64_t n, const int64_t *table_ids,
                              const uint32_t *table_pos, const int64_t *dead, int32_t n_dead, int64_t *out, hipStream_t s);
// key[p] = keys[i] for every live row p that carries id ids[i] (scope_lookup's search); *n_set (device, zeroed by the caller)
// counts the entries that named a live row.
hipError_t launch_keys_scatter(const int64_t *table_ids, const uint32_t *table_pos, int64_t n_rows, const int64_t *ids, const int64_t *keys,
                               int64_t n, const int64_t *dead, int32_t n_dead, int64_t *key, unsigned long long *n_set, hipStream_t s);
// new_key[g][d] for d < n_new = old_key[g][d] for d < first, old_key[g][src[d - first]] beyond, ORR_KEY_NONE when that source is
// negative (a new row): n_cols columns in one launch (the pointer arrays are device memory).  No column aliases its source.
hipError_t launch_keys_remap(const int64_t *src, int64_t first, int64_t n_new, const int64_t *const *old_key, int64_t *const *new_key,
                             int32_t n_cols, hipStream_t s);
// key[0 .. n) = ORR_KEY_NONE
hipError_t launch_keys_fill_none(int64_t *key, int64_t n, hipStream_t s);
// *out (device, zeroed by the caller) += the rows r < n_rows with a key that are not in dead[] (ascending).
hipError_t launch_keys_count(const int64_t *key, int64_t n_rows, const int64_t *dead, int32_t n_dead, unsigned long long *out, hipStream_t s);

// ---- key groups (orr_keys_groups, orr_keys_centroids, orr_scope_centroid; the rules are orr_key_groups_plan.h's) ---------------
// workgroups (and entries of counts / offsets, without the closing one) of launch_keys_pairs over n_rows rows
inline int64_t key_groups_pair_blocks(int64_t n_rows) { return (n_rows + 255) / 256; }
// The selected rows of bm (words * 32 bits, bits at or above n_rows clear) as pairs in candidate order.  mode 0: rows with a key,
// out_key = key_groups::sort_key(key); mode 1: rows whose norm participates and whose key is in tab_keys [n_tab] (ascending,
// distinct), out_key = the key's index in the table; mode 2: rows whose norm participates, positions only.  write false: the
// count pass, counts[key_groups_pair_blocks(n_rows)] written; write true: the pairs stored from offsets[] (the exclusive scan of
// the counts) on, below cap.  No atomics.
hipError_t launch_keys_pairs(int32_t mode, bool write, const int64_t *key, const double *norm_b, int64_t n_rows, const uint32_t *bm, int64_t words,
                             const int64_t *tab_keys, int32_t n_tab, uint32_t *counts, const uint32_t *offsets, int64_t cap, uint64_t *out_key,
                             uint32_t *out_pos, hipStream_t s);
// hipCUB behind the pairs (temp NULL: temp_bytes is set): the exclusive scan of n counts; the stable radix sort of n pairs on the
// key bits [0, end_bit); the runs of the sorted keys (run_key / run_len [n] at most, *n_runs their number).  n < 2^31.
hipError_t keys_pairs_scan(void *temp, size_t &temp_bytes, const uint32_t *counts, uint32_t *offsets, int64_t n, hipStream_t s);
hipError_t keys_pairs_sort(void *temp, size_t &temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *pos_in, uint32_t *pos_out,
                           int64_t n, int32_t end_bit, hipStream_t s);
hipError_t keys_pairs_runs(void *temp, size_t &temp_bytes, const uint64_t *key_sorted, uint64_t *run_key, uint32_t *run_len, uint32_t *n_runs,
                           int64_t n, hipStream_t s);
// One workgroup per block: the fp64 sums of rows emb[pos[first .. first + len)] (positions below n_rows), in this order from
// +0.0, into row `slot` of sums [.][dim] (part == key_groups::kDirect) or row `part` of parts [.][dim].
hipError_t launch_keys_block_sums(const float *emb, int64_t n_rows, int32_t dim, const uint32_t *pos, const key_groups::Block *blocks,
                                  int64_t n_blocks, double *sums, double *parts, hipStream_t s);
// sums[slot] = +0.0 + parts[part0] + ... + parts[part0 + n_blocks - 1], in this order, for each of the n_folds keys.
hipError_t launch_keys_block_fold(const key_groups::Fold *folds, int64_t n_folds, const double *parts, int32_t dim, double *sums, hipStream_t s);
// keys_centroid_finish (orr_keys_centroid_index; the rules are orr_centroid_index_plan.h's): out[i][0 .. dim) =
// key_groups::finish_one(sums[kept[i].slot][.], kept[i].n) and out_ticks[i] = created[pos[kept[i].first]] for the n_kept kept keys
// of a slice, densely.  Every kept[i].n > 0, every kept[i].first a pair of pos, every position of pos a row of created.
hipError_t launch_keys_centroid_finish(const double *sums, int32_t dim, const centroid_index::Kept *kept, int64_t n_kept, const uint32_t *pos,
                                       const int64_t *created, float *out /* [n_kept][dim] */, int64_t *out_ticks /* [n_kept] */, hipStream_t s);
// orr_index_get_rows: out_pos[i] = the position of the first live row with id ids[i] (launch_keys_gather's lookup through the id
// table), found[i] = 1; kRowsFindNone and 0 when there is none.  n_rows < kRowsFindNone.
constexpr uint32_t kRowsFindNone = 0xFFFFFFFFu;
hipError_t launch_rows_find(const int64_t *table_ids, const uint32_t *table_pos, int64_t n_rows, const int64_t *ids, int64_t n, const int64_t *dead,
                            int32_t n_dead, uint32_t *out_pos, uint8_t *found, hipStream_t s);
// keys_chain_step: one workgroup per Chain record and 1,024 coordinates.  The record's key continues on this shard from its state
// rows (S: row 2 * state, P: row 2 * state + 1 of state [.][dim]): the head fragment pos[head_first .. + head_len) on top of the
// carried P, the closed blocks (the head's, then rows part0 .. part0 + n_close - 1 of parts) on top of the carried S, in this
// order; S and the open block's partial are written back (cluster_key_groups::Chain says it add for add).
hipError_t launch_keys_chain_step(const float *emb, int64_t n_rows, int32_t dim, const uint32_t *pos, const cluster_key_groups::Chain *chains,
                                  int64_t n_chains, const double *parts, double *state, hipStream_t s);

// ---- term scopes (orr_scope_create_terms; the rules are orr_scope_terms_plan.h's) -------------------------------------------
// term_base[t] (device, and its copy term_base_host in pinned memory when given) = where distinct term t's row bitmap starts, in
// words from the keyword chain's bitmaps: term_word_off[t] where the alias stage ran (KwView::term_word_off, device; a stored
// token bitmap for an aliased term), t * words where it did not (term_word_off NULL).  1 <= n <= scope_terms::kMaxTerms.
hipError_t launch_scope_terms_bases(const int64_t *term_word_off, int32_t n, int64_t words, int64_t *term_base, int64_t *term_base_host,
                                    hipStream_t s);
// dst (words, all written) = the words of the n distinct terms' bitmaps (bitmaps + term_base[t], read-only: a base may point into
// the stored token bitmaps) folded with AND (scope_terms::All) or OR (Any), the bits at or above n_rows clear.  words % 4 == 0,
// bitmaps and dst 16-byte aligned and every base a multiple of 4 words: one 16-byte load per term and lane.
hipError_t launch_scope_terms_combine(const uint32_t *bitmaps, const int64_t *term_base /* device, [n] words from bitmaps */,
                                      int32_t n, int32_t mode, int64_t words, int64_t n_rows, uint32_t *dst, hipStream_t s);

// ---- cosine scopes (orr_scope_create_near; the rules are orr_scope_near_plan.h's) -------------------------------------------
// bm (words, all written) = bit r set iff row r < n_rows is In or Pending by scope_near::row_state over the device's cosines of
// the nq probes Q [nq][D] with row r of E (exact dots by launch_dot_exact's walk, norm_a [nq] and norm_b [n_rows] the exact
// norms).  Every band pair of a pending row bumps *band_cnt (zeroed by the caller) and, below band_cap, is stored in band.
// 1 <= nq <= kMaxExactQ, D > 0, words % 4 == 0, n_rows <= 32 * words, band 16-byte and bm 8-byte aligned.
hipError_t launch_scope_near(const float *E, int64_t n_rows, int32_t D, const float *Q, int32_t nq, const double *norm_a, const double *norm_b,
                             double min_cosine, int32_t mode, scope_near::BandEntry *band, unsigned long long *band_cnt, int64_t band_cap,
                             uint32_t *bm, int64_t words, hipStream_t s);
// out[i] = norm_b[band[i].pos] for the n entries a walk listed.
hipError_t launch_scope_near_band_norms(const scope_near::BandEntry *band, int64_t n, const double *norm_b, int64_t n_rows, double *out, hipStream_t s);

// ---- cosine range search (orr_search_range_cosine; the rules are orr_range_plan.h's) ----------------------------------------
// The screen: one launch of K2i's 128-row-unit form with the RANGE ending for nq = 1..kMaxI8ScreenQ queries (orr_screen.hip).
hipError_t launch_screen_gemv_i8_range(const void *q1, const void *q2, const float *s1, const double *err2, int32_t nq, const void *tiled,
                                       const float *scale, const float *rel_err, const float *rel_hat, const double *norm_b, int64_t n_rows,
                                       int32_t D, const QueryConst *qc, const double *min_cosine, const uint32_t *allowed, uint32_t *cnt,
                                       SelEntry *buf, uint32_t cap, hipStream_t s);
// The same screen for any number of queries through the int8 screening GEMM's 16 x 16 x 64 form (orr_search_range_cosine_bulk);
// the ONE-level query error bounds it.  args_ws: kRangeTile16ArgsBytes of device memory for the launch.  See orr_screen.hip.
constexpr size_t kRangeTile16ArgsBytes = 128;
hipError_t launch_screen_tile16_range(const void *q_tiled, const float *s1, const double *err2_level1, int32_t nq, const void *e_tiled,
                                      const float *scale, const float *rel_err, const float *rel_hat, const double *norm_b, int64_t n_rows,
                                      int32_t D, const QueryConst *qc, const double *min_cosine, const uint32_t *allowed, uint32_t *cnt,
                                      SelEntry *buf, uint32_t cap, uint32_t *tickets, void *args_ws, hipStream_t s);
// Behind launch_rescore_buffer_exact: every survivor buf[b][i], i < min(cnt[b], cap), of the nq queries with its exact dot
// buf_dot[b][i]: the device's cosine (scope_near::cosine_of), range::device_keeps, and the kept pairs appended to list[b][..]
// (list_cap entries per query, list_cnt [nq] zeroed by the caller counts every kept pair).
hipError_t launch_range_collect(const SelEntry *buf, const double *buf_dot, const uint32_t *cnt, uint32_t cap, int32_t nq, const double *norm_a,
                                const double *norm_b, const int64_t *row_ids, int64_t n_rows, const double *min_cosine,
                                range::ListEntry *list, uint32_t *list_cnt, uint32_t list_cap, hipStream_t s);
// The exact form: the same for EVERY allowed row from dense exact dots dots[q][r] (launch_dot_exact, stride dot_stride).
hipError_t launch_range_collect_dense(const double *dots, int64_t dot_stride, int32_t nq, const double *norm_a, const double *norm_b,
                                      const int64_t *row_ids, int64_t n_rows, const uint32_t *allowed, const double *min_cosine,
                                      range::ListEntry *list, uint32_t *list_cnt, uint32_t list_cap, hipStream_t s);

// ---- diverse search (orr_search_batch_diverse, orr_index_pair_dots; the rules are orr_diverse_plan.h's) ----------------------
// out[l][i][j] = out[l][j][i] = the exact dot (products rounded to binary32, summed in binary64 in index order) of rows
// pos[l][i] and pos[l][j] of E for i, j < cnt[l]; the diagonal is a row's self-dot.  Elements at or beyond cnt[l] are neither
// read nor written.  D > 0, 0 <= cnt[l] <= stride <= diverse::kMaxPool, every listed position below n_rows (the caller's duty:
// a position at or above n_rows is treated as a zero row, never read).  One workgroup per list: any number of lists.
hipError_t launch_pair_dots(const float *E, int64_t n_rows, int32_t D, const uint32_t *pos /* [n_lists][stride] */,
                            const uint32_t *cnt /* [n_lists] */, int32_t n_lists, int32_t stride, double *out /* [n_lists][stride][stride] */,
                            hipStream_t s);

// ---- the cluster's pair step (orr_cluster_search_batch_diverse, orr_cluster_pair_dots; the plan is orr_cluster_diverse_plan.h's)
// launch_pair_dots with two sources: slot i of list l reads row pos[l][i] of the dense buffer F ([n_foreign][D]) where bit i of
// foreign[l] is set, and row pos[l][i] of E otherwise.  A row at or above n_foreign (n_rows) is treated as a zero row, never
// read.  The sums are launch_pair_dots's: a pair's dot does not depend on where its rows lie.
hipError_t launch_pair_dots_two(const float *E, int64_t n_rows, const float *F, int64_t n_foreign, int32_t D,
                                const uint32_t *pos /* [n_lists][stride] */, const uint32_t *cnt /* [n_lists] */,
                                const unsigned long long *foreign /* [n_lists] */, int32_t n_lists, int32_t stride,
                                double *out /* [n_lists][stride][stride] */, hipStream_t s);
// out[i][0 .. D) = E[pos[i]][0 .. D), i < n: the rows a shard sends to other shards, dense.  A position at or above n_rows is
// never read: zeros are written.  D > 0.
hipError_t launch_rows_gather(const float *E, int64_t n_rows, int32_t D, const uint32_t *pos /* [n] */, int64_t n, float *out /* [n][D] */,
                              hipStream_t s);

}  // namespace orr
