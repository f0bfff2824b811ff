// orr_kernels.hip -- gfx950 (CDNA4, wave64) kernels of the hybrid recall-search scorer.
//
// Reference arithmetic being reproduced (src/OmniRecall.Api/Services/RecallSearchService.cs):
//   :77-82  dot/norm sums: float*float rounded to binary32, widened, added to a
//           binary64 accumulator in index order
//   :84-87  guards, dot / (sqrt(normA) * sqrt(normB))
//   :111-112 keyword matches / terms
//   :117-118 exp(-max(0, ageDays) / 30)
//   :66     (cos*0.7) + (kw*0.2) + (rec*0.1), left to right
//   :34-36  order by score desc, CreatedAt desc, stable  == (score desc, candidate
//           position asc) because rows are stored CreatedAt-descending
//
// Built with -ffp-contract=off: nothing here may be fused or re-associated.
#include "orr_kernels.h"
#include "orr_device.h"

#include <hipcub/hipcub.hpp>

#include <cstdlib>

namespace orr {

__global__ __launch_bounds__(256) void row_consts_kernel(const double *__restrict__ norm_b,
                                                         const int64_t *__restrict__ created, int64_t now_ticks,
                                                         int64_t n_rows, double2 *__restrict__ out)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
        out[r] = row_consts_of(norm_b[r], created[r], now_ticks);
    }
}

// Query norms computed on the device (queries that already live there): fills the norm-dependent fields of the
// per-query constants exactly as the host does for host-resident queries.
__global__ void patch_query_norms_kernel(QueryConst *__restrict__ qc, const double *__restrict__ norm_a, int32_t B, int32_t batched,
                                         double *__restrict__ norm_host, const QueryConst *__restrict__ qc_host, double tiny_below)
{
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double na = norm_a[b];
    QueryConst c = qc_host ? qc_host[b] : qc[b];          // (qc_host: the host's copy in pinned memory, read in place -- no upload command)
    c.norm_a = na;
    if (norm_host) norm_host[b] = na;                     // (pinned host memory: no copy command behind this launch)
    if (batched && c.use_cos) {
        if (na <= 0.0) c.use_cos = 0;                     // guard :84 -> cosine 0 for every row
        else c.inv_sqrt_na = 1.0 / sqrt(na);              // NaN stays NaN
        if (na > 0.0 && na < tiny_below) c.use_cos |= kQueryKeepAll;   // (see kQueryKeepAll; tiny_below 0: the pass has no use for it)
    }
    qc[b] = c;
}

hipError_t launch_patch_query_norms(QueryConst *qc, const double *norm_a, int32_t B, bool batched, hipStream_t s, double *norm_host,
                                    const QueryConst *qc_host, double tiny_below)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(patch_query_norms_kernel, dim3((B + 255) / 256), dim3(256), 0, s, qc, norm_a, B, batched ? 1 : 0, norm_host, qc_host,
                       tiny_below);
    return hipGetLastError();
}

hipError_t launch_row_consts(const double *norm_b, const int64_t *created, int64_t now_ticks, int64_t n_rows,
                             double2 *out, hipStream_t s)
{
    if (n_rows <= 0) return hipSuccess;
    int64_t blocks = (n_rows + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(row_consts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, norm_b, created, now_ticks, n_rows, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// K0 / K1e  exact dot: one row per lane, rows staged through a wave-private
// LDS tile so that HBM reads stay coalesced (4 rows x 256 B per wave
// instruction) while each lane walks its own row in index order.
//
// Tile: [64 rows][64 floats] = 16 KiB per wave, 16-byte chunks XOR-swizzled by
// (row & 15) so that the 16-lane groups of ds_read_b128 hit 16 distinct slots.
// ---------------------------------------------------------------------------
// The walk: each wave of the workgroup takes groups of 64 consecutive rows (group g = rows [64 g, 64 g + 64), grid-stride over
// n_groups) and calls end(row0, lane, acc) once per group with acc[q] of lane l = the exact dot of row row0 + l with Q[q]
// (SELF: with itself), 0 for a row at or above n_rows.  dot_exact_tiled and scope_near_tiled are this walk with two endings.
template <int NQ, bool SELF, bool PREFETCH, bool NT, class END>
__device__ __forceinline__ void exact_walk_tiled(const float *E, int64_t n_rows, int64_t n_groups, int32_t D, const float *Q, END end)
{
    __shared__ __attribute__((aligned(16))) float tile_all[4][64 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *tile = tile_all[wave];
    const int ld_row = lane >> 4;     // 0..3: row within a 4-row load
    const int ld_ch = lane & 15;      // 16-byte chunk within the 256-byte row piece

    for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_groups; g += (int64_t)gridDim.x * 4) {
        const int64_t row0 = g << 6;
        double acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = 0.0;

        // global -> registers: 16 wave instructions of 4 rows x 256 B each
        auto load_stage = [&](float4 (&st)[16], int c0) {
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int r = it * 4 + ld_row;
                const int64_t row = row0 + r;
                st[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < n_rows) {
                    const float *src = E + row * (int64_t)D + c0 + ld_ch * 4;
                    if (NT) {   // streamed once: keep it out of the caches
                        typedef float f32x4 __attribute__((ext_vector_type(4)));
                        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(src));
                        st[it] = make_float4(v.x, v.y, v.z, v.w);
                    } else {
                        st[it] = *reinterpret_cast<const float4 *>(src);
                    }
                }
            }
        };
        float4 stage[16];
        if (PREFETCH) load_stage(stage, 0);

        for (int c0 = 0; c0 < D; c0 += 64) {
            if (!PREFETCH) load_stage(stage, c0);
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                const int r = it * 4 + ld_row;
                *reinterpret_cast<float4 *>(tile + r * 64 + ((ld_ch ^ (r & 15)) << 2)) = stage[it];
            }
            // next piece of the rows goes in flight while this one is consumed from LDS
            if (PREFETCH && c0 + 64 < D) load_stage(stage, c0 + 64);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float4 e = *reinterpret_cast<const float4 *>(tile + lane * 64 + ((j ^ (lane & 15)) << 2));
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    float x0, x1, x2, x3;
                    if (SELF) {
                        x0 = e.x; x1 = e.y; x2 = e.z; x3 = e.w;
                    } else {
                        const float *qp = Q + (int64_t)q * D + c0 + j * 4;   // wave-uniform: scalar loads
                        x0 = qp[0]; x1 = qp[1]; x2 = qp[2]; x3 = qp[3];
                    }
                    float p0 = x0 * e.x;
                    acc[q] += (double)p0;
                    float p1 = x1 * e.y;
                    acc[q] += (double)p1;
                    float p2 = x2 * e.z;
                    acc[q] += (double)p2;
                    float p3 = x3 * e.w;
                    acc[q] += (double)p3;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        end(row0, lane, acc);
    }
}

template <int NQ, bool SELF, bool PREFETCH, bool NT>
__global__ __launch_bounds__(256) void dot_exact_tiled(const float *__restrict__ E, int64_t n_rows, int32_t D,
                                                       const float *__restrict__ Q, double *__restrict__ out,
                                                       int64_t out_stride)
{
    exact_walk_tiled<NQ, SELF, PREFETCH, NT>(E, n_rows, (n_rows + 63) >> 6, D, Q, [&](int64_t row0, int lane, const double (&acc)[NQ]) {
        if (row0 + lane < n_rows) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) out[(int64_t)q * out_stride + row0 + lane] = acc[q];
        }
    });
}

// Any D (tests use 2, 3, ...): one thread per row, plain loads.  Correctness path
// for dimensions the tiled kernel does not take (D % 64 != 0).
template <bool SELF>
__global__ __launch_bounds__(256) void dot_exact_generic(const float *__restrict__ E, int64_t n_rows, int32_t D,
                                                         const float *__restrict__ Q, int32_t nq,
                                                         double *__restrict__ out, int64_t out_stride)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const float *e = E + row * (int64_t)D;
    const int nqq = SELF ? 1 : nq;
    for (int q = 0; q < nqq; ++q) {
        const float *x = SELF ? e : Q + (int64_t)q * D;
        double acc = 0.0;
        for (int i = 0; i < D; ++i) {
            float p = x[i] * e[i];
            acc += (double)p;
        }
        out[(int64_t)q * out_stride + row] = acc;
    }
}

hipError_t launch_dot_exact(const float *E, int64_t n_rows, int32_t D, const float *Q, int32_t nq,
                            bool self_norm, double *out, int64_t out_stride, hipStream_t s)
{
    if (n_rows <= 0 || D <= 0) return hipSuccess;
    if (nq < 1 || nq > kMaxExactQ) return hipErrorInvalidValue;
    const bool tiled = (D % 64 == 0) && ((reinterpret_cast<uintptr_t>(E) & 15) == 0);
    if (!tiled) {
        const int64_t blocks = (n_rows + 255) / 256;
        if (self_norm)
            hipLaunchKernelGGL(dot_exact_generic<true>, dim3((unsigned)blocks), dim3(256), 0, s, E, n_rows, D, Q, 1, out, out_stride);
        else
            hipLaunchKernelGGL(dot_exact_generic<false>, dim3((unsigned)blocks), dim3(256), 0, s, E, n_rows, D, Q, nq, out, out_stride);
        return hipGetLastError();
    }
    const int64_t n_groups = (n_rows + 63) / 64;
    int64_t blocks = (n_groups + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;                               // 16 workgroups per CU, grid-stride beyond that (measured best of 2..16)
    dim3 grid((unsigned)blocks), block(256);
    // (register prefetch of the next piece + non-temporal loads: the fastest of the three forms measured in round 1)
#define ORR_LAUNCH_DOT(NQ_, SELF_) hipLaunchKernelGGL((dot_exact_tiled<NQ_, SELF_, true, true>), grid, block, 0, s, E, n_rows, D, Q, out, out_stride)
    if (self_norm) {
        ORR_LAUNCH_DOT(1, true);
    } else {
        switch (nq) {
        case 1: ORR_LAUNCH_DOT(1, false); break;
        case 2: ORR_LAUNCH_DOT(2, false); break;
        case 3: ORR_LAUNCH_DOT(3, false); break;
        case 4: ORR_LAUNCH_DOT(4, false); break;
        case 5: ORR_LAUNCH_DOT(5, false); break;
        case 6: ORR_LAUNCH_DOT(6, false); break;
        case 7: ORR_LAUNCH_DOT(7, false); break;
        default: ORR_LAUNCH_DOT(8, false); break;
        }
    }
#undef ORR_LAUNCH_DOT
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// K3  keyword scan.  Device content pool layout (built at append): every row
// starts on a 16-byte boundary and is followed by 1..16 space bytes up to the next
// boundary.  Query terms never contain whitespace (they come out of a whitespace
// split, RecallSearchService.cs:95), so no term can match across a row boundary
// and only whole lanes past the row end have to be masked.
//
// One wave per row; per step each lane owns 16 consecutive content bytes and the
// 16 four-byte windows starting in them (v_alignbyte), computed once and reused
// for every term.  A term costs one v_cmp per start position (its lane mask is
// OR-ed in scalar registers); terms longer than 4 bytes are verified byte-wise
// only where their 4-byte prefix hit.
// ---------------------------------------------------------------------------
// Tells the compiler a value is the same in every lane (it then lives in SGPRs).
__device__ __forceinline__ int uniform32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uniform64(int64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <bool FULL_MASK>
__device__ __forceinline__ unsigned long long prefix_hits(const uint32_t (&win)[16], uint32_t prefix, uint32_t mask)
{
    unsigned long long any = 0ull;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t v = FULL_MASK ? win[i] : (win[i] & mask);
        any |= __ballot(v == prefix);
    }
    return any;
}

__global__ __launch_bounds__(256) void keyword_scan_kernel(const uint8_t *__restrict__ pool,
                                                           const uint64_t *__restrict__ cstart,
                                                           const uint32_t *__restrict__ clen, int64_t n_rows,
                                                           const uint8_t *__restrict__ term_pool,
                                                           const ScanTerm *__restrict__ terms, int32_t n_terms,
                                                           const uint32_t *__restrict__ q_term_off, int32_t B,
                                                           uint16_t *__restrict__ matches, int64_t matches_stride,
                                                           int32_t accumulate, int32_t group_terms)
{
    // group_terms > 0 (vocabulary form): blockIdx.y selects a group of single-term "queries"; n_terms is the
    // total, q_term_off the identity table 0..group_terms
    if (group_terms > 0) {
        const int32_t first = (int32_t)blockIdx.y * group_terms;
        terms += first;
        matches += (int64_t)first * matches_stride;
        n_terms = n_terms - first < group_terms ? n_terms - first : group_terms;
        B = n_terms;
    }
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = (int64_t)blockIdx.x * 4 + uniform32((int)(threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * 4;

    for (int64_t row = wave_id; row < n_rows; row += n_waves) {
        const uint64_t start = (uint64_t)uniform64((int64_t)cstart[row]);    // 16-byte aligned
        const int len = uniform32((int)clen[row]);
        unsigned long long found = 0ull;                      // wave-uniform bit per term

        for (int cb = 0; cb < len; cb += 1024) {
            const uint8_t *p = pool + start + cb + lane * 16;
            const uint4 w = *reinterpret_cast<const uint4 *>(p);
            const uint32_t w4 = *reinterpret_cast<const uint32_t *>(p + 16);
            uint32_t win[16];
            win[0] = w.x;  win[1] = __builtin_amdgcn_alignbyte(w.y, w.x, 1);
            win[2] = __builtin_amdgcn_alignbyte(w.y, w.x, 2);  win[3] = __builtin_amdgcn_alignbyte(w.y, w.x, 3);
            win[4] = w.y;  win[5] = __builtin_amdgcn_alignbyte(w.z, w.y, 1);
            win[6] = __builtin_amdgcn_alignbyte(w.z, w.y, 2);  win[7] = __builtin_amdgcn_alignbyte(w.z, w.y, 3);
            win[8] = w.z;  win[9] = __builtin_amdgcn_alignbyte(w.w, w.z, 1);
            win[10] = __builtin_amdgcn_alignbyte(w.w, w.z, 2); win[11] = __builtin_amdgcn_alignbyte(w.w, w.z, 3);
            win[12] = w.w; win[13] = __builtin_amdgcn_alignbyte(w4, w.w, 1);
            win[14] = __builtin_amdgcn_alignbyte(w4, w.w, 2);  win[15] = __builtin_amdgcn_alignbyte(w4, w.w, 3);
            // lanes whose 16 bytes begin inside the row (later lanes hold padding or the next row)
            const int live = (len - cb + 15) >> 4;
            const unsigned long long live_mask = live >= 64 ? ~0ull : ((1ull << live) - 1ull);

            for (int t = 0; t < n_terms; ++t) {
                if ((found >> t) & 1ull) continue;
                const ScanTerm tm = terms[t];
                if (tm.len == 0 || (int)tm.len > len) continue;
                unsigned long long any = (tm.mask == 0xFFFFFFFFu) ? prefix_hits<true>(win, tm.prefix, tm.mask)
                                                                  : prefix_hits<false>(win, tm.prefix, tm.mask);
                any &= live_mask;
                if (any == 0ull) continue;
                if (tm.len <= 4) { found |= (1ull << t); continue; }
                // rare: the 4-byte prefix hit somewhere in this step; verify the tail where it hit
                bool hit = false;
                const int pos0 = cb + lane * 16;
                for (int i = 0; i < 16; ++i) {
                    const int pos = pos0 + i;
                    if (win[i] == tm.prefix && pos + (int)tm.len <= len) {
                        bool ok = true;
                        for (uint32_t k = 4; k < tm.len; ++k)
                            ok = ok && (pool[start + pos + k] == term_pool[tm.off + k]);
                        hit = hit || ok;
                    }
                }
                if (__any(hit)) found |= (1ull << t);
            }
        }
        if (lane < B) {
            const uint32_t t0 = q_term_off[lane], t1 = q_term_off[lane + 1];
            unsigned long long m = found >> t0;
            const uint32_t nt = t1 - t0;
            if (nt < 64) m &= ((1ull << nt) - 1ull);
            uint16_t *dst = matches + (int64_t)lane * matches_stride + row;
            *dst = (uint16_t)((accumulate ? *dst : 0) + __popcll(m));
        }
    }
}

hipError_t launch_keyword_scan(const uint8_t *pool, const uint64_t *cstart, const uint32_t *clen, int64_t n_rows,
                               const uint8_t *term_pool, const ScanTerm *terms, int32_t n_terms,
                               const uint32_t *q_term_off, int32_t B, uint16_t *matches,
                               int64_t matches_stride, int32_t accumulate, hipStream_t s)
{
    if (n_rows <= 0 || B <= 0) return hipSuccess;
    if (n_terms > kMaxScanTerms || B > 64) return hipErrorInvalidValue;
    int64_t blocks = (n_rows + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(keyword_scan_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pool, cstart, clen, n_rows, term_pool,
                       terms, n_terms, q_term_off, B, matches, matches_stride, accumulate, 0);
    return hipGetLastError();
}

// Vocabulary form: every one of n_terms distinct terms is its own single-term query; vmatch[t][v] = 1 iff
// term t occurs inside token v.  All groups of kMaxScanTerms terms run in ONE launch (grid.y), which matters
// when the vocabulary is small and a launch is mostly latency.  identity = {0, 1, ..., kMaxScanTerms}.
hipError_t launch_vocab_scan(const uint8_t *vpool, const uint64_t *vstart, const uint32_t *vlen, int64_t n_tokens,
                             const uint8_t *term_pool, const ScanTerm *terms, int32_t n_terms, const uint32_t *identity,
                             uint16_t *vmatch, hipStream_t s)
{
    if (n_tokens <= 0 || n_terms <= 0) return hipSuccess;
    const int32_t groups = (n_terms + kMaxScanTerms - 1) / kMaxScanTerms;
    if (groups > 65535) return hipErrorInvalidValue;
    int64_t blocks = (n_tokens + 3) / 4;
    const int64_t cap = std::max<int64_t>(64, (256 * 8) / groups);
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(keyword_scan_kernel, dim3((unsigned)blocks, (unsigned)groups), dim3(256), 0, s, vpool, vstart, vlen, n_tokens,
                       term_pool, terms, n_terms, identity, 0, vmatch, n_tokens, 0, kMaxScanTerms);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Token index, query side.  The scan kernel above is run over the VOCABULARY
// (one "row" per distinct token of the shard) with one single-term "query" per
// distinct query term: vmatch[t][v] = 1 iff term t occurs inside token v.  A
// whitespace-free term occurs in a row's content iff it occurs inside one of the
// row's whitespace-delimited tokens, so OR-ing the posting lists of the matching
// tokens gives exactly `contentLower.Contains(term)` (RecallSearchService.cs:111)
// for every row.
//
// vocab_hits: one thread per (token, term); every hit reserves its slot in the hit
// list and its run of 1024-posting chunks with ONE 64-bit atomic (count in the high
// word, chunks in the low word), so hit order and chunk order agree.
// expand_hits: grid-stride over chunks; binary search for the owning hit, then 64
// postings per step, one atomicOr each into the term's row bitmap.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vocab_hits_kernel(const uint16_t *__restrict__ vmatch, int64_t n_tokens,
                                                         int32_t n_terms, const uint32_t *__restrict__ token_ids,
                                                         const uint64_t *__restrict__ post_off,
                                                         unsigned long long *__restrict__ counter,
                                                         KwHit *__restrict__ hits, uint32_t max_hits)
{
    const int64_t total = n_tokens * (int64_t)n_terms;
    for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
        if (vmatch[id] == 0) continue;                       // vmatch is [term][token]
        const int64_t t = id / n_tokens;
        int64_t v = id - t * n_tokens;
        if (token_ids) v = token_ids[v];                     // the scanned rows were a subset of the vocabulary
        const uint64_t p0 = post_off[v], p1 = post_off[v + 1];
        const uint32_t chunks = (uint32_t)((p1 - p0 + kPostChunk - 1) / kPostChunk);
        const unsigned long long old = atomicAdd(counter, (1ull << 32) | chunks);
        const uint32_t slot = (uint32_t)(old >> 32);
        if (slot < max_hits) {
            KwHit h;
            h.post_begin = p0; h.post_len = (uint32_t)(p1 - p0); h.chunk_base = (uint32_t)old; h.term = (uint32_t)t; h.token = (uint32_t)v;
            hits[slot] = h;
        }
    }
}

// One thread per hit: how many hits each distinct term has, and (for the terms with one) which token it was.
__global__ __launch_bounds__(256) void kw_term_hits_kernel(const KwHit *__restrict__ hits, const unsigned long long *__restrict__ counter,
                                                           uint32_t max_hits, uint32_t *__restrict__ term_cnt, uint32_t *__restrict__ term_tok)
{
    uint32_t n_hits = (uint32_t)(*counter >> 32);
    if (n_hits > max_hits) n_hits = max_hits;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_hits; i += gridDim.x * blockDim.x) {
        const KwHit h = hits[i];
        atomicAdd(&term_cnt[h.term], 1u);
        term_tok[h.term] = h.token;                    // (the only writer where the count ends up 1)
    }
}

__global__ __launch_bounds__(256) void kw_alias_kernel(const uint32_t *__restrict__ term_cnt, const uint32_t *__restrict__ term_tok,
                                                       const int32_t *__restrict__ tok_bm_index, int32_t n_terms, int64_t bm_store_delta,
                                                       int64_t words_per_term, int64_t *__restrict__ term_word_off, uint8_t *__restrict__ alias)
{
    const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_terms) return;
    int32_t bm = -1;
    if (term_cnt[t] == 1u && tok_bm_index) bm = tok_bm_index[term_tok[t]];
    alias[t] = bm >= 0 ? 1 : 0;
    term_word_off[t] = bm >= 0 ? bm_store_delta + (int64_t)bm * words_per_term : (int64_t)t * words_per_term;
}

// Both steps in ONE workgroup for the few terms of a small batch (a one-query call pays every launch boundary of the keyword
// chain in front of its stream): the counts live in LDS.
constexpr int kKwAliasSmall = 512;
__global__ __launch_bounds__(256) void kw_alias_small_kernel(const KwHit *__restrict__ hits, const unsigned long long *__restrict__ counter,
                                                             uint32_t max_hits, const int32_t *__restrict__ tok_bm_index, int32_t n_terms,
                                                             int64_t bm_store_delta, int64_t words_per_term,
                                                             int64_t *__restrict__ term_word_off, uint8_t *__restrict__ alias)
{
    __shared__ uint32_t cnt[kKwAliasSmall], tok[kKwAliasSmall];
    for (int t = threadIdx.x; t < n_terms; t += blockDim.x) { cnt[t] = 0u; tok[t] = 0u; }
    __syncthreads();
    uint32_t n_hits = (uint32_t)(*counter >> 32);
    if (n_hits > max_hits) n_hits = max_hits;
    for (uint32_t i = threadIdx.x; i < n_hits; i += blockDim.x) {
        const KwHit h = hits[i];
        atomicAdd(&cnt[h.term], 1u);
        tok[h.term] = h.token;                         // (the only writer where the count ends up 1)
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n_terms; t += blockDim.x) {
        int32_t bm = -1;
        if (cnt[t] == 1u && tok_bm_index) bm = tok_bm_index[tok[t]];
        alias[t] = bm >= 0 ? 1 : 0;
        term_word_off[t] = bm >= 0 ? bm_store_delta + (int64_t)bm * words_per_term : (int64_t)t * words_per_term;
    }
}

hipError_t launch_kw_alias(const KwHit *hits, const unsigned long long *counter, uint32_t max_hits, int32_t n_terms,
                           const int32_t *tok_bm_index, int64_t bm_store_delta, int64_t words_per_term, uint32_t *term_cnt,
                           uint32_t *term_tok, int64_t *term_word_off, uint8_t *alias, hipStream_t s)
{
    if (n_terms <= 0) return hipSuccess;
    if (n_terms <= 64) {                               // (a handful of queries: beyond, many workgroups count the hits faster)
        hipLaunchKernelGGL(kw_alias_small_kernel, dim3(1), dim3(256), 0, s, hits, counter, max_hits, tok_bm_index, n_terms, bm_store_delta,
                           words_per_term, term_word_off, alias);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(kw_term_hits_kernel, dim3(64), dim3(256), 0, s, hits, counter, max_hits, term_cnt, term_tok);
    hipLaunchKernelGGL(kw_alias_kernel, dim3((unsigned)((n_terms + 255) / 256)), dim3(256), 0, s, term_cnt, term_tok, tok_bm_index, n_terms,
                       bm_store_delta, words_per_term, term_word_off, alias);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void expand_hits_kernel(const KwHit *__restrict__ hits,
                                                          const unsigned long long *__restrict__ counter,
                                                          uint32_t max_hits, const uint32_t *__restrict__ post_rows,
                                                          uint32_t *__restrict__ bitmaps, int64_t words_per_term,
                                                          unsigned long long *__restrict__ counter_host, const uint8_t *__restrict__ skip_term)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long cnt = *counter;
    if (counter_host && blockIdx.x == 0 && threadIdx.x == 0) *counter_host = cnt;      // statistics (pinned host memory)
    uint32_t n_hits = (uint32_t)(cnt >> 32);
    if (n_hits > max_hits) n_hits = max_hits;       // overflow is detected and retried by the host
    const uint32_t n_chunks = (uint32_t)cnt;
    const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    // a wave takes a CONTIGUOUS run of chunks: one binary search for the hit of its first chunk, a walk along the list for the
    // others (chunk numbers ascend with the hits) -- a fresh search per chunk was fifteen dependent loads each
    const uint32_t per_wave = (n_chunks + n_waves - 1) / n_waves;
    const uint32_t c_first = wave_id * per_wave, c_end = c_first + per_wave < n_chunks ? c_first + per_wave : n_chunks;
    uint32_t lo = 0;
    if (c_first < c_end) {
        uint32_t hi = n_hits;                        // last hit with chunk_base <= c_first
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (hits[mid].chunk_base <= c_first) lo = mid; else hi = mid;
        }
    }
    for (uint32_t c = c_first; c < c_end; ++c) {
        while (lo + 1 < n_hits && hits[lo + 1].chunk_base <= c) ++lo;
        const KwHit h = hits[lo];
        if (skip_term && skip_term[h.term]) continue;   // the term's bitmap is a stored token bitmap: nothing to expand
        const uint64_t post_end = h.post_begin + h.post_len;
        const uint64_t b0 = h.post_begin + (uint64_t)(c - h.chunk_base) * kPostChunk;
        const uint64_t b1 = b0 + kPostChunk < post_end ? b0 + kPostChunk : post_end;
        uint32_t *bm = bitmaps + (int64_t)h.term * words_per_term;
        // posting rows ascend, so the lanes that hit one bitmap word are neighbours: OR their bits
        // together (segmented, 5 steps: a word has 32 bits) and let the last lane of each run do the atomic
        // (four groups of 64 postings in flight: a one-query search has a handful of chunks, each a chain of
        // load -> atomic round trips otherwise)
        for (uint64_t p0 = b0; p0 < b1; p0 += 256) {
            uint32_t rows4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint64_t p = p0 + (uint64_t)g * 64 + lane;
                rows4[g] = p < b1 ? post_rows[p] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t row = rows4[g];
                const bool live = row != 0xFFFFFFFFu;
                const uint32_t word = row >> 5;
                uint32_t bits = live ? 1u << (row & 31) : 0u;
#pragma unroll
                for (int d = 1; d < 32; d <<= 1) {
                    const uint32_t ow = (uint32_t)__shfl_up((int)word, d, 64), ob = (uint32_t)__shfl_up((int)bits, d, 64);
                    if (lane >= d && ow == word) bits |= ob;
                }
                const uint32_t nw = (uint32_t)__shfl_down((int)word, 1, 64);
                if (live && (lane == 63 || nw != word)) atomicOr(&bm[word], bits);
            }
        }
    }
}

hipError_t launch_vocab_hits(const uint16_t *vmatch, int64_t n_tokens, int32_t n_terms, const uint32_t *token_ids,
                             const uint64_t *post_off, unsigned long long *counter, KwHit *hits, uint32_t max_hits, hipStream_t s)
{
    if (n_tokens <= 0 || n_terms <= 0) return hipSuccess;
    int64_t blocks = (n_tokens * (int64_t)n_terms + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(vocab_hits_kernel, dim3((unsigned)blocks), dim3(256), 0, s, vmatch, n_tokens, n_terms, token_ids, post_off,
                       counter, hits, max_hits);
    return hipGetLastError();
}

// Vocabulary tokens of at most 16 bytes (all but URLs and the like): ONE LANE per token instead of one wave.
// The lane keeps its token's 16 four-byte windows in registers; the terms of the block's group are uniform
// (scalar loads), each as up to four dwords with byte masks.  A term occurs in the token iff at some start i
// with i + len(term) <= len(token) every dword of the term equals the window at i + 4j under its mask; bytes
// past the token are padding and never take part.  A hit reserves its slot like vocab_hits does.
__global__ __launch_bounds__(256) void vocab_match_short_kernel(const uint8_t *__restrict__ vpool,
                                                                const uint64_t *__restrict__ vstart,
                                                                const uint32_t *__restrict__ vlen, int64_t n_tokens,
                                                                const MatchTerm *__restrict__ terms, int32_t n_terms,
                                                                const uint64_t *__restrict__ post_off,
                                                                unsigned long long *__restrict__ counter,
                                                                KwHit *__restrict__ hits, uint32_t max_hits)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t t0 = (int32_t)blockIdx.y * kMatchGroup;
    const int32_t t1 = n_terms < t0 + kMatchGroup ? n_terms : t0 + kMatchGroup;
    int32_t len = 0;
    uint4 w = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
    if (v < n_tokens) {
        const uint32_t l = vlen[v];
        if (l >= 1 && l <= 16) { len = (int32_t)l; w = *reinterpret_cast<const uint4 *>(vpool + vstart[v]); }   // rows start 16-byte aligned
    }
    const uint32_t w4 = 0x20202020u;
    uint32_t win[16];
    win[0] = w.x;  win[1] = __builtin_amdgcn_alignbyte(w.y, w.x, 1);
    win[2] = __builtin_amdgcn_alignbyte(w.y, w.x, 2);  win[3] = __builtin_amdgcn_alignbyte(w.y, w.x, 3);
    win[4] = w.y;  win[5] = __builtin_amdgcn_alignbyte(w.z, w.y, 1);
    win[6] = __builtin_amdgcn_alignbyte(w.z, w.y, 2);  win[7] = __builtin_amdgcn_alignbyte(w.z, w.y, 3);
    win[8] = w.z;  win[9] = __builtin_amdgcn_alignbyte(w.w, w.z, 1);
    win[10] = __builtin_amdgcn_alignbyte(w.w, w.z, 2); win[11] = __builtin_amdgcn_alignbyte(w.w, w.z, 3);
    win[12] = w.w; win[13] = __builtin_amdgcn_alignbyte(w4, w.w, 1);
    win[14] = __builtin_amdgcn_alignbyte(w4, w.w, 2);  win[15] = __builtin_amdgcn_alignbyte(w4, w.w, 3);

    for (int32_t t = t0; t < t1; ++t) {
        const uint32_t tlen = (uint32_t)uniform32((int)terms[t].len);
        if (tlen == 0 || tlen > 16) continue;                     // longer terms only fit longer tokens
        const uint32_t w0 = (uint32_t)uniform32((int)terms[t].w[0]), m0 = (uint32_t)uniform32((int)terms[t].m[0]);
        uint32_t cand = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) cand |= ((win[i] & m0) == w0) ? (1u << i) : 0u;
        const int32_t last = len - (int32_t)tlen;                 // last start that keeps the term inside the token
        cand = last < 0 ? 0u : (cand & ((2u << last) - 1u));
        if (__ballot(cand != 0u) == 0ull) continue;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            if (tlen <= 4u * j) break;
            const uint32_t wj = (uint32_t)uniform32((int)terms[t].w[j]), mj = (uint32_t)uniform32((int)terms[t].m[j]);
#pragma unroll
            for (int i = 0; i + 4 * j < 16; ++i)
                if ((win[i + 4 * j] & mj) != wj) cand &= ~(1u << i);
        }
        if (cand == 0u) continue;
        const uint64_t p0 = post_off[v], p1 = post_off[v + 1];
        const uint32_t chunks = (uint32_t)((p1 - p0 + kPostChunk - 1) / kPostChunk);
        const unsigned long long old = atomicAdd(counter, (1ull << 32) | chunks);
        const uint32_t slot = (uint32_t)(old >> 32);
        if (slot < max_hits) {
            KwHit h;
            h.post_begin = p0; h.post_len = (uint32_t)(p1 - p0); h.chunk_base = (uint32_t)old; h.term = (uint32_t)t; h.token = (uint32_t)v;
            hits[slot] = h;
        }
    }
}

// Many terms (a batch of 256+ queries against a vocabulary of 10^5..10^6 tokens): the all-pairs form above costs tokens x terms
// first-dword compares.  Here the terms are LOOKED UP instead: the host sorts them by their (length-masked) first dword in four
// classes -- 1, 2, 3 and 4+ bytes -- and a lane searches each of its token's 16 windows in each non-empty class (binary search,
// then the run of equal keys), verifying the few candidates like the all-pairs form does.  One hit per (token, term): a start
// only counts if no earlier start of the token matches the term too.
//   lk[0..4] = class boundaries in keys / tidx (class c holds the terms of c + 1 bytes, class 3 those of 4..16 bytes).
__device__ __forceinline__ bool term_at(const uint32_t (&win)[16], int i, const MatchTerm &mt)
{
    // (bytes behind the token are spaces, which no term contains: a start too close to the end fails by itself)
    bool ok = (win[i] & mt.m[0]) == mt.w[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (mt.len > 4u * j) {
            const uint32_t wv = i + 4 * j < 16 ? win[(i + 4 * j) & 15] : 0x20202020u;
            ok = ok && (wv & mt.m[j]) == mt.w[j];
        }
    return ok;
}

__global__ __launch_bounds__(256) void vocab_match_lookup_kernel(const uint8_t *__restrict__ vpool, const uint64_t *__restrict__ vstart,
                                                                 const uint32_t *__restrict__ vlen, int64_t n_tokens,
                                                                 const MatchTerm *__restrict__ terms, const uint32_t *__restrict__ lk,
                                                                 const uint32_t *__restrict__ keys, const uint32_t *__restrict__ tidx,
                                                                 const uint32_t *__restrict__ bloom,
                                                                 const uint64_t *__restrict__ post_off, unsigned long long *__restrict__ counter,
                                                                 KwHit *__restrict__ hits, uint32_t max_hits)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int32_t len = 0;
    uint4 w = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
    if (v < n_tokens) {
        const uint32_t l = vlen[v];
        if (l >= 1 && l <= 16) { len = (int32_t)l; w = *reinterpret_cast<const uint4 *>(vpool + vstart[v]); }   // rows start 16-byte aligned
    }
    const uint32_t w4 = 0x20202020u;
    uint32_t win[16];
    win[0] = w.x;  win[1] = __builtin_amdgcn_alignbyte(w.y, w.x, 1);
    win[2] = __builtin_amdgcn_alignbyte(w.y, w.x, 2);  win[3] = __builtin_amdgcn_alignbyte(w.y, w.x, 3);
    win[4] = w.y;  win[5] = __builtin_amdgcn_alignbyte(w.z, w.y, 1);
    win[6] = __builtin_amdgcn_alignbyte(w.z, w.y, 2);  win[7] = __builtin_amdgcn_alignbyte(w.z, w.y, 3);
    win[8] = w.z;  win[9] = __builtin_amdgcn_alignbyte(w.w, w.z, 1);
    win[10] = __builtin_amdgcn_alignbyte(w.w, w.z, 2); win[11] = __builtin_amdgcn_alignbyte(w.w, w.z, 3);
    win[12] = w.w; win[13] = __builtin_amdgcn_alignbyte(w4, w.w, 1);
    win[14] = __builtin_amdgcn_alignbyte(w4, w.w, 2);  win[15] = __builtin_amdgcn_alignbyte(w4, w.w, 3);
    // a Bloom filter of the (class, key) pairs in LDS (built by the host, kVocabBloomBits bits): sixteen independent reads per class
    // instead of sixteen binary searches of dependent loads; a window goes to the search only when its bit is set
    __shared__ uint32_t bloom_lds[kVocabBloomBits / 32];
    // The hits of a workgroup are staged in LDS and reserved in the global list with ONE atomic (hit slots and posting chunks come
    // out of one 64-bit counter and must stay jointly ascending: expand_hits searches the list by chunk number): a batch of 256
    // queries against 250,000 tokens leaves 23,000 hits, and as many atomics on one address were the whole cost of the all-pairs
    // form (0.27 ms of which 0.02 is comparing).
    constexpr uint32_t kStage = 512;
    __shared__ KwHit staged[kStage];
    __shared__ unsigned long long local_ctr, base_ctr;
    for (int i = threadIdx.x; i < kVocabBloomBits / 32; i += 256) bloom_lds[i] = bloom[i];
    if (threadIdx.x == 0) local_ctr = 0ull;
    __syncthreads();
    if (len != 0) {
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {                                 // (not unrolled: sixteen copies of the search are code enough)
        const uint32_t c0 = lk[c], c1 = lk[c + 1];
        if (c0 == c1) continue;                                   // (uniform: no term of this class in the batch)
        const uint32_t mask = c == 0 ? 0xFFu : c == 1 ? 0xFFFFu : c == 2 ? 0xFFFFFFu : 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i + c + 1 > len) continue;                        // the shortest term of this class does not fit behind this start
            const uint32_t key = win[i] & mask;
            const uint32_t hb = vocab_bloom_hash(key, (uint32_t)c);
            if (!((bloom_lds[hb >> 5] >> (hb & 31u)) & 1u)) continue;
            uint32_t lo = c0, hi = c1;                            // lower bound of key in keys[c0, c1)
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (keys[mid] < key) lo = mid + 1; else hi = mid;
            }
            for (uint32_t pos = lo; pos < c1 && keys[pos] == key; ++pos) {
                const uint32_t t = tidx[pos];
                const MatchTerm mt = terms[t];
                if ((int32_t)mt.len > len - i) continue;          // the term would run past the token's end
                if (!term_at(win, i, mt)) continue;
                bool earlier = false;                             // one hit per (token, term)
                for (int e = 0; e < i; ++e) earlier = earlier || term_at(win, e, mt);
                if (earlier) continue;
                const uint64_t p0 = post_off[v], p1 = post_off[v + 1];
                const uint32_t chunks = (uint32_t)((p1 - p0 + kPostChunk - 1) / kPostChunk);
                KwHit h;
                h.post_begin = p0; h.post_len = (uint32_t)(p1 - p0); h.term = t; h.token = (uint32_t)v;
                const unsigned long long mine = atomicAdd(&local_ctr, (1ull << 32) | chunks);
                if ((uint32_t)(mine >> 32) < kStage) {
                    h.chunk_base = (uint32_t)mine;                // (relative to the workgroup's block: rebased below)
                    staged[(uint32_t)(mine >> 32)] = h;
                } else {                                          // (more hits than the stage holds: straight into the list)
                    const unsigned long long old = atomicAdd(counter, (1ull << 32) | chunks);
                    const uint32_t slot = (uint32_t)(old >> 32);
                    h.chunk_base = (uint32_t)old;
                    if (slot < max_hits) hits[slot] = h;
                }
            }
        }
    }
    }
    __syncthreads();
    // the staged hits: everything up to the first one that did not fit (hits and chunks counted in the order of the local counter)
    const uint32_t n_local = (uint32_t)(local_ctr >> 32) < kStage ? (uint32_t)(local_ctr >> 32) : kStage;
    if (n_local == 0) return;
    if (threadIdx.x == 0) {
        // chunks of the staged hits = the local chunk counter where hit number n_local began (or the total when all fit)
        uint32_t staged_chunks = (uint32_t)local_ctr;
        if ((uint32_t)(local_ctr >> 32) > kStage) {
            const KwHit &last = staged[kStage - 1];
            staged_chunks = last.chunk_base + (uint32_t)((last.post_len + kPostChunk - 1) / kPostChunk);
        }
        base_ctr = atomicAdd(counter, ((unsigned long long)n_local << 32) | staged_chunks);
    }
    __syncthreads();
    const uint32_t base_slot = (uint32_t)(base_ctr >> 32), base_chunk = (uint32_t)base_ctr;
    for (uint32_t i = threadIdx.x; i < n_local; i += 256) {
        KwHit h = staged[i];
        h.chunk_base += base_chunk;
        if (base_slot + i < max_hits) hits[base_slot + i] = h;
    }
}

hipError_t launch_vocab_match_lookup(const uint8_t *vpool, const uint64_t *vstart, const uint32_t *vlen, int64_t n_tokens,
                                     const MatchTerm *terms, const uint32_t *lk, const uint32_t *keys, const uint32_t *tidx,
                                     const uint32_t *bloom, const uint64_t *post_off, unsigned long long *counter, KwHit *hits,
                                     uint32_t max_hits, hipStream_t s)
{
    if (n_tokens <= 0) return hipSuccess;
    const int64_t blocks = (n_tokens + 255) / 256;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vocab_match_lookup_kernel, dim3((unsigned)blocks), dim3(256), 0, s, vpool, vstart, vlen, n_tokens, terms, lk, keys, tidx,
                       bloom, post_off, counter, hits, max_hits);
    return hipGetLastError();
}

// The same for tokens of 17..32 bytes, given as a list (start, length, token number): 32 windows per lane, terms of up to 32
// bytes (eight dwords); longer terms cannot occur in these tokens.
__global__ __launch_bounds__(256) void vocab_match_mid_kernel(const uint8_t *__restrict__ vpool, const uint64_t *__restrict__ starts,
                                                              const uint32_t *__restrict__ lens, const uint32_t *__restrict__ ids,
                                                              int64_t n_list, const MatchTerm8 *__restrict__ terms, int32_t n_terms,
                                                              const uint64_t *__restrict__ post_off, unsigned long long *__restrict__ counter,
                                                              KwHit *__restrict__ hits, uint32_t max_hits)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t t0 = (int32_t)blockIdx.y * kMatchGroup;
    const int32_t t1 = n_terms < t0 + kMatchGroup ? n_terms : t0 + kMatchGroup;
    int32_t len = 0;
    uint32_t v = 0u;
    uint32_t w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = 0x20202020u;
    if (i < n_list) {
        const uint32_t l = lens[i];
        if (l >= 17 && l <= 32) {
            len = (int32_t)l;
            v = ids[i];
            const uint4 a = *reinterpret_cast<const uint4 *>(vpool + starts[i]);            // rows start 16-byte aligned; a token
            const uint4 b = *reinterpret_cast<const uint4 *>(vpool + starts[i] + 16);       // of 17..32 bytes owns at least 32
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        }
    }
    uint32_t win[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        win[4 * k] = w[k];
        win[4 * k + 1] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], 1);
        win[4 * k + 2] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], 2);
        win[4 * k + 3] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], 3);
    }
    for (int32_t t = t0; t < t1; ++t) {
        const uint32_t tlen = (uint32_t)uniform32((int)terms[t].len);
        if (tlen == 0 || tlen > 32) continue;
        const uint32_t w0 = (uint32_t)uniform32((int)terms[t].w[0]), m0 = (uint32_t)uniform32((int)terms[t].m[0]);
        uint32_t cand = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) cand |= ((win[k] & m0) == w0) ? (1u << k) : 0u;
        const int32_t last = len - (int32_t)tlen;                 // last start that keeps the term inside the token (<= 31)
        cand = last < 0 ? 0u : (cand & ((2u << last) - 1u));
        if (__ballot(cand != 0u) == 0ull) continue;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            if (tlen <= 4u * j) break;
            const uint32_t wj = (uint32_t)uniform32((int)terms[t].w[j]), mj = (uint32_t)uniform32((int)terms[t].m[j]);
#pragma unroll
            for (int k = 0; k + 4 * j < 32; ++k)
                if ((win[k + 4 * j] & mj) != wj) cand &= ~(1u << k);
        }
        if (cand == 0u) continue;
        const uint64_t p0 = post_off[v], p1 = post_off[v + 1];
        const uint32_t chunks = (uint32_t)((p1 - p0 + kPostChunk - 1) / kPostChunk);
        const unsigned long long old = atomicAdd(counter, (1ull << 32) | chunks);
        const uint32_t slot = (uint32_t)(old >> 32);
        if (slot < max_hits) {
            KwHit h;
            h.post_begin = p0; h.post_len = (uint32_t)(p1 - p0); h.chunk_base = (uint32_t)old; h.term = (uint32_t)t; h.token = v;
            hits[slot] = h;
        }
    }
}

hipError_t launch_vocab_match_mid(const uint8_t *vpool, const uint64_t *starts, const uint32_t *lens, const uint32_t *ids, int64_t n_list,
                                  const MatchTerm8 *terms, int32_t n_terms, const uint64_t *post_off, unsigned long long *counter,
                                  KwHit *hits, uint32_t max_hits, hipStream_t s)
{
    if (n_list <= 0 || n_terms <= 0) return hipSuccess;
    const int64_t blocks = (n_list + 255) / 256;
    const int32_t groups = (n_terms + kMatchGroup - 1) / kMatchGroup;
    if (groups > 65535 || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vocab_match_mid_kernel, dim3((unsigned)blocks, (unsigned)groups), dim3(256), 0, s, vpool, starts, lens, ids, n_list,
                       terms, n_terms, post_off, counter, hits, max_hits);
    return hipGetLastError();
}

hipError_t launch_vocab_match_short(const uint8_t *vpool, const uint64_t *vstart, const uint32_t *vlen, int64_t n_tokens,
                                    const MatchTerm *terms, int32_t n_terms, const uint64_t *post_off,
                                    unsigned long long *counter, KwHit *hits, uint32_t max_hits, hipStream_t s)
{
    if (n_tokens <= 0 || n_terms <= 0) return hipSuccess;
    const int64_t blocks = (n_tokens + 255) / 256;
    const int32_t groups = (n_terms + kMatchGroup - 1) / kMatchGroup;
    if (groups > 65535 || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(vocab_match_short_kernel, dim3((unsigned)blocks, (unsigned)groups), dim3(256), 0, s, vpool, vstart, vlen,
                       n_tokens, terms, n_terms, post_off, counter, hits, max_hits);
    return hipGetLastError();
}

hipError_t launch_expand_hits(const KwHit *hits, const unsigned long long *counter, uint32_t max_hits,
                              const uint32_t *post_rows, uint32_t *bitmaps, int64_t words_per_term, hipStream_t s,
                              unsigned long long *counter_host, const uint8_t *skip_term)
{
    hipLaunchKernelGGL(expand_hits_kernel, dim3(1024), dim3(256), 0, s, hits, counter, max_hits, post_rows, bitmaps,
                       words_per_term, counter_host, skip_term);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// K4 + K5a  fused score and per-workgroup selection.  One workgroup scans
// kSelSegRows rows of one query: each wave walks a quarter of them 64 at a time
// (lane = row, coalesced 8-byte reads), skips batches that cannot enter its
// list, and the four lists are merged through LDS at the end.
// ---------------------------------------------------------------------------
// LANEMAX (the sampled prefix of a two-stage pass, whose lists only serve the floor): every lane keeps the best of its U rows
// and the wave's list is ONE sort of those -- the k-th best of such maxima belongs to k distinct rows, so it is a valid floor,
// and with thousands of lanes per query it is the k-th best row's key itself unless two of the k best rows share a lane
// (k^2 / (2 x 13,000) of the time at 10M rows): a quarter of the sorts and none of the merges of the full ranking.
// LANEMAX = 2 (enough segments for 8 k wave maxima per query): nothing is sorted at all -- every wave writes the best of its 256 rows
// into slot `wave` of the segment's list (16 entries per list, the rest unused), and the floor is the k-th best of those
// (select_floor_heads_kernel with 16 entries per list).
template <bool FAST, int LANEMAX>
__global__ __launch_bounds__(1024) void fuse_select_kernel(const double *__restrict__ dot,
                                                           const float *__restrict__ dotf, int64_t dot_stride,
                                                           const double *__restrict__ norm_b,
                                                           const int64_t *__restrict__ created,
                                                           const double2 *__restrict__ row_consts, KwView kw,
                                                           const QueryConst *__restrict__ qcs,
                                                           int64_t now_ticks, int64_t n_rows, int32_t seg_first,
                                                           int32_t n_seg_total,
                                                           const unsigned long long *__restrict__ tau,
                                                           SelEntry *__restrict__ out_sel, I8Prefix i8)
{
    __shared__ SelEntry lists[16][kSelWidth];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x;                        // queries vary fastest: neighbouring workgroups share a segment
    const int seg = seg_first + blockIdx.y;
    const QueryConst qc = qcs[b];
    // Rows after the sampled prefix only matter if they beat the k'-th best key of the prefix
    // (equal keys lose the position tie-break to the prefix rows): most batches are skipped.
    const unsigned long long floor_key = tau ? tau[b] : 0ull;
    const int64_t seg0 = (int64_t)seg * kSelSegRows;
    const int64_t seg1 = (seg0 + kSelSegRows < n_rows) ? seg0 + kSelSegRows : n_rows;
    // int8 prefix: the query's part of the per-pair bound, as the screening GEMM's epilogue forms it
    double i8_qs1 = 0.0, i8_qw = 0.0;
    if (FAST && i8.rowf) {
        i8_qs1 = (double)i8.qs1[b];
        i8_qw = qc.use_cos ? (double)__double2float_ru(0.7 * 1.000001 * sqrt(i8.qerr2[b]) * qc.inv_sqrt_na) : 0.0;
    }

    // each of the 16 waves scores kSelSegRows/16 = 256 rows: 4 batches of 64 whose loads are
    // all issued before the first use
    constexpr int U = kSelSegRows / (16 * 64);
    unsigned long long k = 0ull;
    uint32_t p = 0xFFFFFFFFu;
    unsigned long long nk[U];
    uint32_t np[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t r = seg0 + (int64_t)(wave * U + u) * 64 + lane;
        nk[u] = 0ull;
        np[u] = 0xFFFFFFFFu;
        if (r < seg1) {
            const double d = !qc.use_cos ? 0.0
                             : dotf  ? (double)dotf[(int64_t)b * dot_stride + r]     // K2 candidate pass
                                     : dot[(int64_t)b * dot_stride + r];             // K1e exact
            const uint32_t m = qc.n_terms > 0 ? kw_matches(kw, b, (uint32_t)r) : 0u;
            if (FAST && i8.rowf) {
                const double2 rc = row_consts[r];
                const float4 rf = i8.rowf[r];
                const double bound = qc.use_cos ? (double)rf.y + i8_qw * (double)rf.z : 0.0;
                const double sc = fused_score_fast(d * ((double)rf.x * i8_qs1), rc.x, rc.y, m, qc) - bound;
                nk[u] = score_key(sc);
                if (!(fabs(sc) <= 1.7976931348623157e308)) nk[u] = 1ull;          // non-finite: no floor from it
            } else if (FAST) {
                const double2 rc = row_consts[r];
                nk[u] = score_key(fused_score_fast(d, rc.x, rc.y, m, qc));
                // an fp32 sum that overflowed: a ranking keeps the pair for the exact re-score, a floor takes nothing from it
                // (likewise every pair of a query whose products with the rows are subnormal: kQueryKeepAll)
                if (dotf && (dot_overflowed(d, rc.x, qc) || ((qc.use_cos & kQueryKeepAll) && rc.x > 0.0))) nk[u] = LANEMAX ? 1ull : kKeptKey;
            } else {
                nk[u] = score_key(fused_score(d, norm_b[r], created[r], m, qc, now_ticks));
            }
            np[u] = (uint32_t)r;
        }
    }
    if (LANEMAX) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (better(nk[u], np[u], k, p)) { k = nk[u]; p = np[u]; }
        if (LANEMAX == 2) {
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const unsigned long long ok = __shfl_xor(k, d, 64);
                const uint32_t op = __shfl_xor(p, d, 64);
                if (better(ok, op, k, p)) { k = ok; p = op; }
            }
            if (lane == 0) {
                SelEntry e;
                e.key = k; e.pos = p; e.pad = 0;
                out_sel[((int64_t)b * n_seg_total + seg) * kSelWidth + wave] = e;
            }
            return;
        }
        wave_sort(k, p, lane);
    }
#pragma unroll
    for (int u = 0; u < U && LANEMAX == 0; ++u) {
        if (seg0 + (int64_t)(wave * U + u) * 64 >= seg1) break;
        if (floor_key) {
            if (!__any(nk[u] > floor_key)) continue;
            if (nk[u] <= floor_key) { nk[u] = 0ull; np[u] = 0xFFFFFFFFu; }
        }
        const unsigned long long tk = __shfl(k, 63, 64);
        const uint32_t tp = __shfl(p, 63, 64);
        if (!__any(better(nk[u], np[u], tk, tp))) continue;
        wave_sort(nk[u], np[u], lane);
        wave_merge_sorted(k, p, nk[u], np[u], lane);
    }
    lists[wave][lane].key = k;
    lists[wave][lane].pos = p;
    __syncthreads();
#pragma unroll
    for (int stride = 8; stride > 0; stride >>= 1) {
        if (wave < stride) {
            wave_merge_sorted(k, p, lists[wave + stride][lane].key, lists[wave + stride][lane].pos, lane);
            lists[wave][lane].key = k;
            lists[wave][lane].pos = p;
        }
        __syncthreads();
    }
    if (wave == 0) {
        SelEntry e;
        e.key = k; e.pos = p; e.pad = 0;
        out_sel[((int64_t)b * n_seg_total + seg) * kSelWidth + lane] = e;
    }
}

hipError_t launch_fuse_select(const double *dot, const float *dotf, int64_t dot_stride, const double *norm_b,
                              const int64_t *created, const double2 *row_consts, KwView kw,
                              const QueryConst *qc, int64_t now_ticks, int64_t n_rows, int32_t B,
                              int32_t seg_first, int32_t seg_count, const unsigned long long *tau,
                              SelEntry *out_sel, int32_t n_seg_stride, hipStream_t s, I8Prefix i8, int floor_only)
{
    if (n_rows <= 0 || B <= 0 || seg_count <= 0) return hipSuccess;
    const int64_t n_seg = n_seg_stride > 0 ? n_seg_stride : (n_rows + kSelSegRows - 1) / kSelSegRows;
    if (n_seg > 65535) return hipErrorInvalidValue;
    if (floor_only && (tau || !row_consts)) return hipErrorInvalidValue;
    if (floor_only == 2)
        hipLaunchKernelGGL((fuse_select_kernel<true, 2>), dim3((unsigned)B, (unsigned)seg_count), dim3(1024), 0, s, dot, dotf, dot_stride,
                           norm_b, created, row_consts, kw, qc, now_ticks, n_rows, seg_first, (int32_t)n_seg, tau, out_sel, i8);
    else if (floor_only)
        hipLaunchKernelGGL((fuse_select_kernel<true, 1>), dim3((unsigned)B, (unsigned)seg_count), dim3(1024), 0, s, dot, dotf, dot_stride,
                           norm_b, created, row_consts, kw, qc, now_ticks, n_rows, seg_first, (int32_t)n_seg, tau, out_sel, i8);
    else if (row_consts)
        hipLaunchKernelGGL((fuse_select_kernel<true, 0>), dim3((unsigned)B, (unsigned)seg_count), dim3(1024), 0, s, dot, dotf, dot_stride,
                           norm_b, created, row_consts, kw, qc, now_ticks, n_rows, seg_first, (int32_t)n_seg, tau, out_sel, i8);
    else
        hipLaunchKernelGGL((fuse_select_kernel<false, 0>), dim3((unsigned)B, (unsigned)seg_count), dim3(1024), 0, s, dot, dotf, dot_stride,
                           norm_b, created, row_consts, kw, qc, now_ticks, n_rows, seg_first, (int32_t)n_seg, tau, out_sel, I8Prefix());
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// K5b  final merge per query: 16 waves fold the n_seg sorted lists, then a
// 4-level tree through LDS; wave 0 writes kprime records and the trailer.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void select_final_kernel(const SelEntry *__restrict__ sel, int32_t n_seg,
                                                            int32_t seg_stride, int32_t kprime, int64_t n_rows, int64_t row_base,
                                                            const double *__restrict__ dot,
                                                            const float *__restrict__ dotf, int64_t dot_stride,
                                                            const double *__restrict__ norm_b,
                                                            const int64_t *__restrict__ created,
                                                            const int64_t *__restrict__ row_ids, KwView kw,
                                                            int32_t dot_exact, double approx_eps,
                                                            unsigned long long *__restrict__ tau_out,
                                                            const uint32_t *__restrict__ fused_cnt, uint32_t fused_cap,
                                                            const double *__restrict__ two_stage_L,
                                                            orr_candidate *__restrict__ out, FloorOut floor)
{
    __shared__ SelEntry lists[16][kSelWidth];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const SelEntry *mine = sel + (int64_t)b * seg_stride * kSelWidth;

    unsigned long long k = 0ull;
    uint32_t p = 0xFFFFFFFFu;
    constexpr int U = 8;     // lists fetched together
    for (int sg0 = wave; sg0 < n_seg; sg0 += 16 * U) {
        SelEntry e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int sgi = sg0 + 16 * u;
            e[u].key = 0ull; e[u].pos = 0xFFFFFFFFu;
            if (sgi < n_seg) e[u] = mine[(int64_t)sgi * kSelWidth + lane];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (sg0 + 16 * u >= n_seg) break;
            wave_merge_sorted(k, p, e[u].key, e[u].pos, lane);
        }
    }
    lists[wave][lane].key = k;
    lists[wave][lane].pos = p;
    __syncthreads();
#pragma unroll
    for (int stride = 8; stride > 0; stride >>= 1) {
        if (wave < stride) {
            wave_merge_sorted(k, p, lists[wave + stride][lane].key, lists[wave + stride][lane].pos, lane);
            lists[wave][lane].key = k;
            lists[wave][lane].pos = p;
        }
        __syncthreads();
    }
    if (wave == 0 && tau_out) {      // sampling pass: only the k'-th best key of these lists is wanted
        // (of the keys that are scores: pairs kept whatever their score -- kKeptKey, in front of every score -- say nothing about
        // the k'-th best; with fewer than k' scores behind them there is no floor)
        const int n_kept = __popcll(__ballot(k == kKeptKey));
        const unsigned long long kth_any = __shfl(k, (kprime - 1 + n_kept) & 63, 64);
        const unsigned long long kth = kprime - 1 + n_kept < 64 ? kth_any : 0ull;
        if (lane == 0) {
            tau_out[b] = kth;                     // 0 (empty slot) if fewer than k' rows: no filtering
            if (floor.floor_key) two_stage_floor_of(kth, floor.eps3, floor.eps1, floor.floor_key + b, floor.L + b);
        }
        return;
    }
    if (wave == 0) {
        orr_candidate *o = out + (int64_t)b * (kprime + 1);
        if (lane < kprime)
            write_record(o + lane, k, p, b, row_base, dot, dotf, dot_stride, norm_b, created, row_ids, kw, dot_exact);
        const unsigned long long valid_mask = __ballot(k != 0ull && lane < kprime);
        const int n_valid = __popcll(valid_mask);
        const unsigned long long worst_key = __shfl(k, (n_valid > 0 ? n_valid - 1 : 0), 64);
        if (lane == 0) {
            orr_candidate t;
            // two-stage: every buffered row became a record -> the only rows left out are below L
            const bool kept_all = n_rows <= (int64_t)kprime || (two_stage_L && fused_cnt && fused_cnt[b] <= (uint32_t)kprime);
            t.approx_score = (kept_all || n_valid == 0) ? -__builtin_huge_val() : cutoff_of_key(worst_key);
            t.dot = approx_eps; t.norm_b = 0.0; t.created_ticks = 0;
            t.row_id = -1; t.order_key = n_rows; t.matches = n_valid; t.flags = ORR_CAND_TRAILER;
            if (fused_cnt && fused_cnt[b] > fused_cap) t.flags |= ORR_CAND_OVERFLOW;
            if (two_stage_L) { t.norm_b = two_stage_L[b]; t.flags |= ORR_CAND_TWO_STAGE; }
            o[kprime] = t;
        }
    }
}

hipError_t launch_select_final(const SelEntry *sel, int32_t n_seg, int32_t B, int32_t kprime,
                               int64_t n_rows, int64_t row_base, const double *dot, const float *dotf,
                               int64_t dot_stride, const double *norm_b, const int64_t *created,
                               const int64_t *row_ids, KwView kw, int32_t dot_exact, double approx_eps,
                               unsigned long long *tau_out, const uint32_t *fused_cnt, uint32_t fused_cap,
                               const double *two_stage_L, orr_candidate *out, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    if (kprime < 1 || kprime > kSelWidth) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_final_kernel, dim3((unsigned)B), dim3(1024), 0, s, sel, n_seg, n_seg, kprime, n_rows, row_base,
                       dot, dotf, dot_stride, norm_b, created, row_ids, kw, dot_exact, approx_eps, tau_out, fused_cnt, fused_cap, two_stage_L, out, FloorOut());
    return hipGetLastError();
}

// The floor from MANY lists (a one-query call's sampled stream leaves 128 of them): the k-th best of the lists' HEADS belongs to
// k distinct rows, so it is a valid floor, and it is the k-th best row's key unless two of the k best rows share a list
// (k^2 / (2 lists) of the time: the floor is then the (k+1)-th best).  One wave per query instead of sixteen merging every list.
__global__ __launch_bounds__(64) void select_floor_heads_kernel(const SelEntry *__restrict__ sel, int32_t n_seg, int32_t seg_stride,
                                                                int32_t kprime, unsigned long long *__restrict__ tau_out, FloorOut floor,
                                                                int32_t per_list)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    const SelEntry *mine = sel + (int64_t)b * seg_stride * kSelWidth;
    unsigned long long k = 0ull;
    uint32_t p = 0xFFFFFFFFu;
    // per_list = 1: the heads of sorted lists; 16: the 16 wave maxima a floor-only ranking left in each list's first slots
    for (int i = lane; i < n_seg * per_list; i += 64) {
        const SelEntry e = mine[(int64_t)(i / per_list) * kSelWidth + (i % per_list)];
        if (better(e.key, e.pos, k, p)) { k = e.key; p = e.pos; }
    }
    wave_sort(k, p, lane);
    // (heads that are no scores -- kKeptKey -- are passed over: the k-th best of the others still belongs to k distinct rows)
    const int n_kept = __popcll(__ballot(k == kKeptKey));
    const unsigned long long kth_any = __shfl(k, (kprime - 1 + n_kept) & 63, 64);
    const unsigned long long kth = kprime - 1 + n_kept < 64 ? kth_any : 0ull;
    if (lane == 0) {
        tau_out[b] = kth;
        if (floor.floor_key) two_stage_floor_of(kth, floor.eps3, floor.eps1, floor.floor_key + b, floor.L + b);
    }
}

hipError_t launch_select_final_sample(const SelEntry *sel, int32_t n_seg_total, int32_t sample_seg, int32_t B,
                                      int32_t kprime, unsigned long long *tau_out, hipStream_t s, FloorOut floor, int32_t wave_maxima,
                                      int32_t merge_all)
{
    if (B <= 0 || sample_seg <= 0) return hipSuccess;
    if (kprime < 1 || kprime > kSelWidth) return hipErrorInvalidValue;
    if (wave_maxima) {                                                 // (the lists hold 16 wave maxima each: fuse_select's LANEMAX = 2)
        if (!floor.floor_key) return hipErrorInvalidValue;
        hipLaunchKernelGGL(select_floor_heads_kernel, dim3((unsigned)B), dim3(64), 0, s, sel, sample_seg, n_seg_total, kprime, tau_out, floor, 16);
        return hipGetLastError();
    }
    static const bool full = getenv("ORR_FLOOR_FULL") != nullptr;      // (A/B)
    if (floor.floor_key && sample_seg >= 8 * kprime && !full && !merge_all) {        // (a two-stage pass's floor: any k distinct rows' k-th key serves)
        hipLaunchKernelGGL(select_floor_heads_kernel, dim3((unsigned)B), dim3(64), 0, s, sel, sample_seg, n_seg_total, kprime, tau_out, floor, 1);
        return hipGetLastError();
    }
    const KwView nokw{nullptr, 0, nullptr, nullptr};
    hipLaunchKernelGGL(select_final_kernel, dim3((unsigned)B), dim3(1024), 0, s, sel, sample_seg, n_seg_total, kprime,
                       (int64_t)0, (int64_t)0, nullptr, nullptr, (int64_t)0, nullptr, nullptr, nullptr, nokw, 0, 0.0,
                       tau_out, nullptr, 0u, nullptr, nullptr, floor);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Generic large-k path: all keys -> stable descending radix sort -> records.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_keys_kernel(const double *__restrict__ dot,
                                                         const double *__restrict__ norm_b,
                                                         const int64_t *__restrict__ created, KwView kw, int32_t b,
                                                         QueryConst qc, int64_t now_ticks, int64_t n_rows,
                                                         unsigned long long *__restrict__ keys,
                                                         uint32_t *__restrict__ vals)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
        const double d = qc.use_cos ? dot[r] : 0.0;
        const uint32_t m = qc.n_terms > 0 ? kw_matches(kw, b, (uint32_t)r) : 0u;
        keys[r] = score_key(fused_score(d, norm_b[r], created[r], m, qc, now_ticks));
        vals[r] = (uint32_t)r;
    }
}

hipError_t launch_score_keys(const double *dot, const double *norm_b, const int64_t *created,
                             KwView kw, int32_t b, QueryConst qc, int64_t now_ticks, int64_t n_rows,
                             unsigned long long *keys, uint32_t *vals, hipStream_t s)
{
    if (n_rows <= 0) return hipSuccess;
    int64_t blocks = (n_rows + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(score_keys_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dot, norm_b, created, kw, b, qc,
                       now_ticks, n_rows, keys, vals);
    return hipGetLastError();
}

hipError_t sort_pairs_desc(void *temp, size_t &temp_bytes, const unsigned long long *keys_in,
                           unsigned long long *keys_out, const uint32_t *vals_in, uint32_t *vals_out,
                           int64_t n, hipStream_t s)
{
    return hipcub::DeviceRadixSort::SortPairsDescending(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out,
                                                        (int)n, 0, 64, s);
}

__global__ __launch_bounds__(256) void records_from_sorted_kernel(const unsigned long long *__restrict__ keys,
                                                                  const uint32_t *__restrict__ vals, int32_t K,
                                                                  int64_t n_rows, int64_t row_base,
                                                                  const double *__restrict__ dot, int64_t dot_stride,
                                                                  const double *__restrict__ norm_b,
                                                                  const int64_t *__restrict__ created,
                                                                  const int64_t *__restrict__ row_ids, KwView kw,
                                                                  int32_t b, int32_t dot_exact,
                                                                  orr_candidate *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < K) {
        if ((int64_t)i < n_rows)
            write_record(out + i, keys[i], vals[i], b, row_base, dot, nullptr, dot_stride, norm_b, created, row_ids, kw, dot_exact);
        else
            write_record(out + i, 0ull, 0u, b, row_base, dot, nullptr, dot_stride, norm_b, created, row_ids, kw, dot_exact);
    } else if (i == K) {
        orr_candidate t;
        const int64_t n_valid = n_rows < (int64_t)K ? n_rows : (int64_t)K;
        const bool kept_all = n_rows <= (int64_t)K;
        t.approx_score = (kept_all || n_valid == 0) ? -__builtin_huge_val() : key_score(keys[n_valid - 1]);
        t.dot = 0.0; t.norm_b = 0.0; t.created_ticks = 0;
        t.row_id = -1; t.order_key = n_rows; t.matches = (int32_t)n_valid; t.flags = ORR_CAND_TRAILER;
        out[K] = t;
    }
}

hipError_t launch_records_from_sorted(const unsigned long long *keys, const uint32_t *vals, int32_t K,
                                      int64_t n_rows, int64_t row_base, const double *dot, int64_t dot_stride,
                                      const double *norm_b, const int64_t *created, const int64_t *row_ids,
                                      KwView kw, int32_t b, int32_t dot_exact, orr_candidate *out,
                                      hipStream_t s)
{
    const int blocks = (K + 1 + 255) / 256;
    hipLaunchKernelGGL(records_from_sorted_kernel, dim3(blocks), dim3(256), 0, s, keys, vals, K, n_rows, row_base, dot,
                       dot_stride, norm_b, created, row_ids, kw, b, dot_exact, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Seal-time permutation into candidate order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_f32_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                              const int64_t *__restrict__ perm, int64_t n, int32_t D)
{
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const float *s = src + perm[r] * (int64_t)D;
        float *d = dst + r * (int64_t)D;
        for (int i = threadIdx.x; i < D; i += blockDim.x) d[i] = s[i];
    }
}

__global__ __launch_bounds__(256) void gather_i64_kernel(const int64_t *__restrict__ src, int64_t *__restrict__ dst,
                                                         const int64_t *__restrict__ perm, int64_t n)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        dst[r] = src[perm[r]];
}

// dst row r <- src row perm[r] (perm == nullptr: identity).  Source rows are
// (src_start, len) byte ranges; destination rows start at dst_start[r].
__global__ __launch_bounds__(256) void gather_content_kernel(const uint8_t *__restrict__ src_pool,
                                                             const uint64_t *__restrict__ src_start,
                                                             const uint32_t *__restrict__ src_len,
                                                             uint8_t *__restrict__ dst_pool,
                                                             const uint64_t *__restrict__ dst_start,
                                                             const int64_t *__restrict__ perm, int64_t n)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave_id; r < n; r += n_waves) {
        const int64_t sr = perm ? perm[r] : r;
        const uint64_t s0 = src_start[sr], d0 = dst_start[r];
        const uint32_t len = src_len[sr];
        for (uint32_t i = lane; i < len; i += 64) dst_pool[d0 + i] = src_pool[s0 + i];
    }
}

__global__ __launch_bounds__(256) void gather_u32_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                         const int64_t *__restrict__ perm, int64_t n)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        dst[r] = src[perm[r]];
}

// ---- orr_index_insert_rows: the two-source row merge.  Destination row r takes E row src_idx[r] when that is >= 0, else row
// ~src_idx[r] - stage_base of the staging buffer (the new rows of this round).  One wave per row; whole rows move as 16-byte
// vectors when D % 4 == 0 (four in flight per lane), element by element otherwise.  E and dst may be the SAME array (rows
// moving up inside the shard): the caller guarantees that no source row of a launch lies inside its destination range.
__global__ __launch_bounds__(256) void merge_rows_f32_kernel(const float *E, const float *stage, const int64_t *__restrict__ src_idx,
                                                             int64_t stage_base, float *dst, int64_t n, int32_t D)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave_id; r < n; r += n_waves) {
        const int64_t si = src_idx[r];
        const float *s = si >= 0 ? E + si * (int64_t)D : stage + (~si - stage_base) * (int64_t)D;
        float *d = dst + r * (int64_t)D;
        if ((D & 3) == 0) {
            const float4 *s4 = reinterpret_cast<const float4 *>(s);
            float4 *d4 = reinterpret_cast<float4 *>(d);
            const int32_t n4 = D >> 2;
            int32_t i = lane;
            for (; i + 192 < n4; i += 256) {
                const float4 a = s4[i], b = s4[i + 64], c = s4[i + 128], e = s4[i + 192];
                d4[i] = a; d4[i + 64] = b; d4[i + 128] = c; d4[i + 192] = e;
            }
            for (; i < n4; i += 64) d4[i] = s4[i];
        } else {
            for (int32_t i = lane; i < D; i += 64) d[i] = s[i];
        }
    }
}

// the same choice for one 8-byte value per row (timestamps, ids, norms as bit patterns); add[] is indexed by ~src_idx[r]
__global__ __launch_bounds__(256) void merge_i64_kernel(const int64_t *__restrict__ old, const int64_t *__restrict__ add,
                                                        const int64_t *__restrict__ src_idx, int64_t *__restrict__ dst, int64_t n)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t si = src_idx[r];
        dst[r] = si >= 0 ? old[si] : add[~si];
    }
}

// ---- deleted rows (orr_index_delete_rows).  A deleted row keeps its position; its norm and timestamp are
// overwritten so that it scores at most 0.2 (keyword part only) and its records are flagged for the host
// finish, which drops them.
__global__ void tombstone_rows_kernel(const int64_t *pos, int32_t n, double *norm_b, int64_t *created)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    norm_b[pos[i]] = 0.0;          // cosine 0 through the norm guard (:84)
    created[pos[i]] = 0;           // year 1: exp(-age / 30) underflows to 0
}

__global__ void mark_dead_records_kernel(orr_candidate *recs, int64_t count, int32_t stride, const int64_t *dead,
                                         int32_t n_dead, int64_t row_base)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || (int32_t)(i % stride) == stride - 1) return;     // trailers stay as they are
    const int64_t key = recs[i].order_key;
    if (recs[i].row_id < 0 && key < 0) return;
    const int64_t p = key - row_base;
    int32_t lo = 0, hi = n_dead;                                       // dead[] ascending
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (dead[mid] < p) lo = mid + 1; else hi = mid;
    }
    if (lo < n_dead && dead[lo] == p) recs[i].flags |= ORR_CAND_DEAD;
}

__global__ __launch_bounds__(256) void iota_i64_kernel(int64_t *__restrict__ dst, int64_t n, int64_t base)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        dst[r] = base + r;
}

static inline unsigned capped_blocks(int64_t work_items, int per_block)
{
    int64_t b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > 256 * 8) b = 256 * 8;
    return (unsigned)b;
}

hipError_t launch_gather_rows_f32(const float *src, float *dst, const int64_t *perm, int64_t n, int32_t D, hipStream_t s)
{
    if (n <= 0 || D <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_f32_kernel, dim3(capped_blocks(n, 1)), dim3(256), 0, s, src, dst, perm, n, D);
    return hipGetLastError();
}

hipError_t launch_gather_i64(const int64_t *src, int64_t *dst, const int64_t *perm, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_i64_kernel, dim3(capped_blocks(n, 256)), dim3(256), 0, s, src, dst, perm, n);
    return hipGetLastError();
}

hipError_t launch_merge_rows_f32(const float *E, const float *stage, const int64_t *src_idx, int64_t stage_base, float *dst,
                                 int64_t n, int32_t D, hipStream_t s)
{
    if (n <= 0 || D <= 0) return hipSuccess;
    // one wave per row up to 2^20 workgroups (a chunk of 256 MiB has fewer rows than that for D >= 64): a capped grid would
    // give some waves one row more than others, a tenth of the launch's time at 12 KB rows
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)1 << 20);
    hipLaunchKernelGGL(merge_rows_f32_kernel, dim3(blocks), dim3(256), 0, s, E, stage, src_idx, stage_base, dst, n, D);
    return hipGetLastError();
}

hipError_t launch_merge_i64(const int64_t *old, const int64_t *add, const int64_t *src_idx, int64_t *dst, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(merge_i64_kernel, dim3(capped_blocks(n, 256)), dim3(256), 0, s, old, add, src_idx, dst, n);
    return hipGetLastError();
}

hipError_t launch_gather_content(const uint8_t *src_pool, const uint64_t *src_start, const uint32_t *src_len,
                                 uint8_t *dst_pool, const uint64_t *dst_start, const int64_t *perm, int64_t n,
                                 hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_content_kernel, dim3(capped_blocks(n, 4)), dim3(256), 0, s, src_pool, src_start, src_len,
                       dst_pool, dst_start, perm, n);
    return hipGetLastError();
}

hipError_t launch_gather_u32(const uint32_t *src, uint32_t *dst, const int64_t *perm, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_u32_kernel, dim3(capped_blocks(n, 256)), dim3(256), 0, s, src, dst, perm, n);
    return hipGetLastError();
}

hipError_t launch_iota_i64(int64_t *dst, int64_t n, int64_t base, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(iota_i64_kernel, dim3(capped_blocks(n, 256)), dim3(256), 0, s, dst, n, base);
    return hipGetLastError();
}

hipError_t launch_tombstone_rows(const int64_t *pos, int32_t n, double *norm_b, int64_t *created, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(tombstone_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pos, n, norm_b, created);
    return hipGetLastError();
}

hipError_t launch_mark_dead_records(orr_candidate *recs, int32_t B, int32_t kprime, const int64_t *dead, int32_t n_dead,
                                    int64_t row_base, hipStream_t s)
{
    const int64_t count = (int64_t)B * (kprime + 1);
    if (count <= 0 || n_dead <= 0) return hipSuccess;
    hipLaunchKernelGGL(mark_dead_records_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, recs, count, kprime + 1,
                       dead, n_dead, row_base);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Scoped search (orr_search_batch_scoped): the rows a caller lists by id become the entries of the survivors' buffers
// the exact tail of the two-stage pass consumes.  No kernel here reads an embedding of a row outside a scope.
//   id table     the shard's (row id, position) pairs sorted by id: ids[] ascending, pos[] ascending within equal ids
//   bitmaps      one bit per row of the shard and scope: removes repeats, keeps candidate order, and makes candidate_limit a
//                prefix popcount (scope::clip_word, shared with the host's selftest)
//   chunks       kScopeChunkWords words of a bitmap: the unit of the popcounts and of the compaction's workgroups
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iota_u32_kernel(uint32_t *__restrict__ dst, int64_t n)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) dst[r] = (uint32_t)r;
}

hipError_t scope_sort_id_table(void *temp, size_t &temp_bytes, const int64_t *ids_in, int64_t *ids_out, uint32_t *pos_in,
                               uint32_t *pos_out, int64_t n, hipStream_t s)
{
    if (temp) {
        hipLaunchKernelGGL(iota_u32_kernel, dim3(capped_blocks(n, 256)), dim3(256), 0, s, pos_in, n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // (a stable radix sort: equal ids keep their positions ascending)
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, ids_in, ids_out, pos_in, pos_out, (int)n, 0, 64, s);
}

// One thread per listed id: the run of equal ids in the table, every live position of it a bit in the bitmap of the query that
// owns the id (scope_off[n_q + 1] relative to ids[0]; null: one bitmap for all).  Unknown ids find no run.
__global__ __launch_bounds__(256) void scope_lookup_kernel(const int64_t *__restrict__ table_ids, const uint32_t *__restrict__ table_pos,
                                                           int64_t n_rows, const int64_t *__restrict__ ids, int64_t n_ids,
                                                           const uint64_t *__restrict__ scope_off, int32_t n_q,
                                                           const int64_t *__restrict__ dead, int32_t n_dead,
                                                           uint32_t *__restrict__ bitmaps, int64_t words)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ids) return;
    int64_t bm = 0;
    if (scope_off) {                                   // the query b with scope_off[b] <= i < scope_off[b + 1]
        int32_t lo = 0, hi = n_q;
        while (hi - lo > 1) {
            const int32_t mid = (lo + hi) >> 1;
            if (scope_off[mid] <= (uint64_t)i) lo = mid; else hi = mid;
        }
        bm = lo;
    }
    const int64_t want = ids[i];
    int64_t lo = 0, hi = n_rows;                       // first table entry with id >= want
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (table_ids[mid] < want) lo = mid + 1; else hi = mid;
    }
    for (; lo < n_rows && table_ids[lo] == want; ++lo) {
        const uint32_t p = table_pos[lo];
        int32_t dl = 0, dh = n_dead;                   // deleted rows take no part (dead[] ascending)
        while (dl < dh) {
            const int32_t mid = (dl + dh) >> 1;
            if (dead[mid] < (int64_t)p) dl = mid + 1; else dh = mid;
        }
        if (dl < n_dead && dead[dl] == (int64_t)p) continue;
        atomicOr(bitmaps + bm * words + (p >> 5), 1u << (p & 31u));
    }
}

hipError_t launch_scope_lookup(const int64_t *table_ids, const uint32_t *table_pos, int64_t n_rows, const int64_t *ids, int64_t n_ids,
                               const uint64_t *scope_off, int32_t n_q, const int64_t *dead, int32_t n_dead, uint32_t *bitmaps,
                               int64_t words, hipStream_t s)
{
    if (n_ids <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(scope_lookup_kernel, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, s, table_ids, table_pos, n_rows, ids, n_ids,
                       scope_off, n_q, dead, n_dead, bitmaps, words);
    return hipGetLastError();
}

__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t *sh4)   // 256 threads; every thread gets the sum
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    __syncthreads();                                   // (sh4 may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}

// chunk_cnt[bm][chunk] = set bits of that chunk
__global__ __launch_bounds__(256) void scope_chunk_counts_kernel(const uint32_t *__restrict__ bitmaps, int64_t words, int32_t n_chunks,
                                                                 uint32_t *__restrict__ chunk_cnt)
{
    __shared__ uint32_t sh4[4];
    const int64_t bm = blockIdx.x, w0 = (int64_t)blockIdx.y * kScopeChunkWords + (int64_t)threadIdx.x * 4;
    uint32_t c = 0;
    if (w0 < words) {                                  // (words is a multiple of 4: whole uint4s)
        const uint4 v = *reinterpret_cast<const uint4 *>(bitmaps + bm * words + w0);
        c = __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    c = block_sum_u32(c, sh4);
    if (threadIdx.x == 0) chunk_cnt[bm * n_chunks + blockIdx.y] = c;
}

// Per query: live[q] = rows its scope resolves to, took[q] = min(live, limit[q]) (either may be pinned host memory)
__global__ __launch_bounds__(256) void scope_totals_kernel(const uint32_t *__restrict__ chunk_cnt, int32_t n_chunks, int32_t shared_scope,
                                                           const int64_t *__restrict__ limit, uint32_t *__restrict__ live,
                                                           uint32_t *__restrict__ took)
{
    __shared__ uint32_t sh4[4];
    const int q = blockIdx.x;
    const uint32_t *mine = chunk_cnt + (int64_t)(shared_scope ? 0 : q) * n_chunks;
    uint32_t c = 0;
    for (int i = threadIdx.x; i < n_chunks; i += 256) c += mine[i];
    c = block_sum_u32(c, sh4);
    if (threadIdx.x == 0) {
        live[q] = c;
        const int64_t lim = limit[q] < 0 ? 0 : limit[q];
        took[q] = (int64_t)c < lim ? c : (uint32_t)lim;
    }
}

hipError_t launch_scope_counts(const uint32_t *bitmaps, int64_t words, int32_t n_bitmaps, int32_t n_q, const int64_t *limit,
                               uint32_t *chunk_cnt, uint32_t *live, uint32_t *took, hipStream_t s)
{
    if (n_q <= 0 || n_bitmaps <= 0) return hipSuccess;
    if (words % 4 != 0 || (n_bitmaps != 1 && n_bitmaps != n_q)) return hipErrorInvalidValue;
    const int32_t n_chunks = scope_chunks(words);
    if (n_chunks > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_chunk_counts_kernel, dim3((unsigned)n_bitmaps, (unsigned)n_chunks), dim3(256), 0, s, bitmaps, words, n_chunks, chunk_cnt);
    hipLaunchKernelGGL(scope_totals_kernel, dim3((unsigned)n_q), dim3(256), 0, s, chunk_cnt, n_chunks, n_bitmaps == 1 && n_q > 1 ? 1 : 0, limit,
                       live, took);
    return hipGetLastError();
}

// Workgroup (i, chunk): query qsel[i] of the slice's bitmaps; the chunk's set bits, clipped to the query's first limit rows,
// become entries buf[i][rank] in candidate order (key 1: a placeholder the re-score overwrites; 0 would be an empty slot).
__global__ __launch_bounds__(256) void scope_compact_kernel(const uint32_t *__restrict__ bitmaps, int64_t words, int32_t n_chunks,
                                                            const uint32_t *__restrict__ chunk_cnt, int32_t shared_scope,
                                                            const uint32_t *__restrict__ qsel, const int64_t *__restrict__ limit,
                                                            SelEntry *__restrict__ buf, uint32_t cap)
{
    __shared__ uint32_t sh4[4];
    __shared__ uint32_t wave_base[4];
    const int i = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = qsel[i];
    const int64_t bm = shared_scope ? 0 : (int64_t)q;
    const uint32_t *cc = chunk_cnt + bm * n_chunks;
    if (cc[chunk] == 0u) return;                                   // (uniform: most chunks of a small scope)
    const int64_t lim = limit[q] < 0 ? 0 : limit[q];
    uint32_t before = 0;                                           // set bits in front of this chunk
    for (int c = tid; c < chunk; c += 256) before += cc[c];
    before = block_sum_u32(before, sh4);
    if ((int64_t)before >= lim) return;
    const int64_t w0 = (int64_t)chunk * kScopeChunkWords + (int64_t)tid * 4;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (w0 < words) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bitmaps + bm * words + w0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    const uint32_t mine = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
    uint32_t incl = mine;                                          // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wave_base[wave] = incl;
    __syncthreads();
    uint32_t rank = before + incl - mine;
    for (int k = 0; k < wave; ++k) rank += wave_base[k];
    SelEntry *out = buf + (int64_t)i * cap;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t bits = scope::clip_word(w[k], (uint64_t)rank, (uint64_t)lim);
        rank += __popc(w[k]);
        uint32_t r = rank - __popc(w[k]);
        while (bits) {
            const uint32_t bit = (uint32_t)__ffs((int)bits) - 1u;
            bits &= bits - 1u;
            if (r < cap) {
                SelEntry e;
                e.key = 1ull; e.pos = (uint32_t)((w0 + k) * 32 + bit); e.pad = 0u;
                out[r] = e;
            }
            ++r;
        }
    }
}

hipError_t launch_scope_compact(const uint32_t *bitmaps, int64_t words, int32_t n_bitmaps, const uint32_t *chunk_cnt, const uint32_t *qsel,
                                int32_t n_sel, const int64_t *limit, SelEntry *buf, uint32_t cap, hipStream_t s)
{
    if (n_sel <= 0) return hipSuccess;
    if (words % 4 != 0 || cap == 0) return hipErrorInvalidValue;
    const int32_t n_chunks = scope_chunks(words);
    if (n_chunks > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_compact_kernel, dim3((unsigned)n_sel, (unsigned)n_chunks), dim3(256), 0, s, bitmaps, words, n_chunks, chunk_cnt,
                       n_bitmaps == 1 ? 1 : 0, qsel, limit, buf, cap);
    return hipGetLastError();
}

// The re-score of the buffered pairs where the tail's own kernels do not apply (a dimension that is no multiple of 64, or no
// cosine at all: dim 0, a query of another dimension): one thread per pair, the reference's sum in index order.
__global__ __launch_bounds__(256) void scope_rescore_generic_kernel(const float *__restrict__ E, int32_t D, const float *__restrict__ Q,
                                                                    const double *__restrict__ norm_b, const int64_t *__restrict__ created,
                                                                    KwView kw, const QueryConst *__restrict__ qcs, int64_t now_ticks,
                                                                    const uint32_t *__restrict__ cnt, uint32_t cap, SelEntry *__restrict__ buf,
                                                                    double *__restrict__ buf_dot)
{
    const int b = blockIdx.x;
    const uint32_t n = cnt[b] < cap ? cnt[b] : cap;
    const QueryConst qc = qcs[b];
    for (uint32_t i = blockIdx.y * 256u + threadIdx.x; i < n; i += gridDim.y * 256u) {
        SelEntry *mine = buf + (int64_t)b * cap + i;
        const int64_t row = (int64_t)mine->pos;
        double acc = 0.0;
        if (qc.use_cos) {
            const float *e = E + row * (int64_t)D, *q = Q + (int64_t)b * D;
            for (int c = 0; c < D; ++c) {
                const float p = q[c] * e[c];
                acc += (double)p;
            }
        }
        const uint32_t m = (qc.n_terms > 0 && kw.bitmaps) ? kw_matches(kw, b, (uint32_t)row) : 0u;
        mine->key = score_key(fused_score(acc, norm_b[row], created[row], m, qc, now_ticks));
        mine->pad = m;
        buf_dot[(int64_t)b * cap + i] = acc;
    }
}

hipError_t launch_scope_rescore_generic(const float *E, int32_t D, const float *Q, int32_t B, const double *norm_b, const int64_t *created,
                                        KwView kw, const QueryConst *qc, int64_t now_ticks, const uint32_t *cnt, uint32_t cap, SelEntry *buf,
                                        double *buf_dot, hipStream_t s)
{
    if (B <= 0 || cap == 0) return hipSuccess;
    const unsigned gy = (unsigned)std::min<uint32_t>((cap + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(scope_rescore_generic_kernel, dim3((unsigned)B, gy), dim3(256), 0, s, E, D, Q, norm_b, created, kw, qc, now_ticks, cnt, cap,
                       buf, buf_dot);
    return hipGetLastError();
}

// AllRecords: every buffered pair a record with its exact dot (buf_dot, written by the re-score), in candidate order; empty
// records behind them; the trailer says that nothing was cut (approx_score -inf) and how many scoped rows took part.
__global__ __launch_bounds__(256) void scope_records_kernel(const SelEntry *__restrict__ buf, const double *__restrict__ buf_dot,
                                                            const uint32_t *__restrict__ cnt, uint32_t cap, int32_t kprime, int64_t row_base,
                                                            const double *__restrict__ norm_b, const int64_t *__restrict__ created,
                                                            const int64_t *__restrict__ row_ids, KwView kw, orr_candidate *__restrict__ recs)
{
    const int b = blockIdx.x;
    const uint32_t n = cnt[b] < cap ? cnt[b] : cap;
    orr_candidate *o = recs + (int64_t)b * ((int64_t)kprime + 1);
    for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i <= (int64_t)kprime; i += (int64_t)gridDim.y * 256) {
        orr_candidate c;
        if (i == (int64_t)kprime) {
            const uint32_t valid = n < (uint32_t)kprime ? n : (uint32_t)kprime;
            c.approx_score = -__builtin_huge_val(); c.dot = 0.0; c.norm_b = 0.0; c.created_ticks = 0;
            c.row_id = -1; c.order_key = (int64_t)n; c.matches = (int32_t)valid; c.flags = ORR_CAND_TRAILER;
        } else if (i < (int64_t)n) {
            const SelEntry e = buf[(int64_t)b * cap + i];
            c.approx_score = key_score(e.key);
            c.dot = buf_dot[(int64_t)b * cap + i];
            c.norm_b = norm_b[e.pos];
            c.created_ticks = created[e.pos];
            c.row_id = row_ids[e.pos];
            c.order_key = row_base + (int64_t)e.pos;
            c.matches = kw.bitmaps ? (int32_t)kw_matches(kw, b, e.pos) : 0;
            c.flags = ORR_CAND_DOT_EXACT;
        } else {
            c.approx_score = 0.0; c.dot = 0.0; c.norm_b = 0.0; c.created_ticks = 0;
            c.row_id = -1; c.order_key = -1; c.matches = 0; c.flags = 0;
        }
        o[i] = c;
    }
}

hipError_t launch_scope_records(const SelEntry *buf, const double *buf_dot, const uint32_t *cnt, uint32_t cap, int32_t B, int32_t kprime,
                                int64_t row_base, const double *norm_b, const int64_t *created, const int64_t *row_ids, KwView kw,
                                orr_candidate *recs, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    if (kprime < 1) return hipErrorInvalidValue;
    const unsigned gy = (unsigned)std::min<int64_t>(((int64_t)kprime + 1 + 255) / 256, 1024);
    hipLaunchKernelGGL(scope_records_kernel, dim3((unsigned)B, gy), dim3(256), 0, s, buf, buf_dot, cnt, cap, kprime, row_base, norm_b, created,
                       row_ids, kw, recs);
    return hipGetLastError();
}

// Selection: the tail's trailers say "two-stage, floor L, n rows took part"; a scoped pass has no floor and its rows are the
// query's scoped ones -- order_key = the scoped rows that took part, no ORR_CAND_TWO_STAGE, norm_b 0.
__global__ void scope_trailers_kernel(orr_candidate *recs, int32_t B, int32_t kprime, const uint32_t *__restrict__ cnt)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    orr_candidate *t = recs + (int64_t)b * ((int64_t)kprime + 1) + kprime;
    t->order_key = (int64_t)cnt[b];
    t->norm_b = 0.0;
    t->flags &= ~ORR_CAND_TWO_STAGE;
}

hipError_t launch_scope_trailers(orr_candidate *recs, int32_t B, int32_t kprime, const uint32_t *cnt, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(scope_trailers_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, recs, B, kprime, cnt);
    return hipGetLastError();
}

// ---- masked search (orr_search_batch_masked; the rules are orr_mask_plan.h's) -----------------------------------------------

// One workgroup of 256: *n_clip = one past the position of the took-th set bit (1 <= took <= set bits) of a bitmap whose chunk
// counts exist.  Thread t sums a contiguous run of chunks, thread 0 walks the 256 sums and then that run; the chunk found is
// scanned the same way, four words per thread; scope::clip_word leaves the took-th bit as the highest of the last word.
// Every thread of the workgroup calls it (it synchronises); the rule of mask_clip_kernel and of group_gather_clip_kernel.
__device__ __forceinline__ void mask_clip_rule(const uint32_t *__restrict__ bitmap, int64_t words, int32_t n_chunks,
                                               const uint32_t *__restrict__ chunk_cnt, uint32_t took, int64_t *__restrict__ n_clip)
{
    __shared__ uint32_t part[256];
    __shared__ int32_t s_at;
    __shared__ uint32_t s_before;
    const int tid = threadIdx.x;
    const int32_t per = (n_chunks + 255) / 256;
    const int32_t c0 = min(n_chunks, tid * per), c1 = min(n_chunks, c0 + per);
    uint32_t sum = 0;
    for (int32_t c = c0; c < c1; ++c) sum += chunk_cnt[c];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t before = 0;
        int t = 0;
        while (t < 255 && before + part[t] < took) before += part[t++];
        int32_t c = min(n_chunks - 1, t * per);
        const int32_t c_end = min(n_chunks, c + per) - 1;
        while (c < c_end && before + chunk_cnt[c] < took) before += chunk_cnt[c++];
        s_at = c; s_before = before;
    }
    __syncthreads();
    const int32_t chunk = s_at;
    const int64_t w0 = (int64_t)chunk * kScopeChunkWords + (int64_t)tid * 4;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (w0 < words) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bitmap + w0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    uint32_t before = s_before;
    __syncthreads();                                   // (part and s_at are written again)
    part[tid] = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        while (t < 255 && before + part[t] < took) before += part[t++];
        s_at = t; s_before = before;
    }
    __syncthreads();
    if (tid != s_at) return;
    before = s_before;
    int64_t clip = words * 32;                         // (took beyond the set bits: every row)
    for (int k = 0; k < 4; ++k) {
        const uint32_t c = __popc(w[k]);
        if (c != 0u && before + c >= took) {
            const uint32_t kept = scope::clip_word(w[k], (uint64_t)before, (uint64_t)took);
            clip = (w0 + k) * 32 + (32 - __clz((int)kept));
            break;
        }
        before += c;
    }
    *n_clip = clip;
}

// Workgroup s clips bitmap s of [gridDim.x][words] (chunk counts [gridDim.x][n_chunks]) into n_clip[s]: one workgroup and `took` for
// launch_mask_clip; for launch_mask_clip_slots took_of[s] (device memory) is the slot's took, and a slot without a set bit gives 0.
__global__ __launch_bounds__(256) void mask_clip_kernel(const uint32_t *__restrict__ bitmap, int64_t words, int32_t n_chunks,
                                                        const uint32_t *__restrict__ chunk_cnt, uint32_t took,
                                                        const uint32_t *__restrict__ took_of, int64_t *__restrict__ n_clip)
{
    const int64_t sl = blockIdx.x;
    if (took_of) {
        took = took_of[sl];                            // (workgroup-uniform)
        if (took == 0u) {
            if (threadIdx.x == 0) n_clip[sl] = 0;
            return;
        }
    }
    mask_clip_rule(bitmap + sl * words, words, n_chunks, chunk_cnt + sl * n_chunks, took, n_clip + sl);
}

hipError_t launch_mask_clip(const uint32_t *bitmap, int64_t words, const uint32_t *chunk_cnt, uint32_t took, int64_t *n_clip, hipStream_t s)
{
    if (words <= 0 || words % 4 != 0 || took == 0u) return hipErrorInvalidValue;
    const int32_t n_chunks = scope_chunks(words);
    hipLaunchKernelGGL(mask_clip_kernel, dim3(1), dim3(256), 0, s, bitmap, words, n_chunks, chunk_cnt, took, (const uint32_t *)nullptr, n_clip);
    return hipGetLastError();
}

// launch_mask_clip for n_slots contiguous bitmaps in ONE launch, took = the slot's set bits (live, device memory): n_clip[s] = one
// past the last set bit of bitmap s, 0 for an empty one (what refresh_scope keeps as a scope's n_clip_all).
hipError_t launch_mask_clip_slots(const uint32_t *bitmaps, int64_t words, const uint32_t *chunk_cnt, const uint32_t *live, int32_t n_slots,
                                  int64_t *n_clip, hipStream_t s)
{
    if (n_slots <= 0) return hipSuccess;
    if (words <= 0 || words % 4 != 0 || !bitmaps || !chunk_cnt || !live || !n_clip) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_clip_kernel, dim3((unsigned)n_slots), dim3(256), 0, s, bitmaps, words, scope_chunks(words), chunk_cnt, 0u, live, n_clip);
    return hipGetLastError();
}

// The front of a grouped pass over scope handles in ONE launch: blockIdx.y = an entry of the table (a used group), the
// workgroups of a row copy the group's bitmap (16 bytes per lane, contiguous per wave, grid-stride) and chunk counts from the
// handle's own arrays into slot `slot` of the call's contiguous arrays; workgroup x == 0 of an entry whose took lies below the
// handle's live rows (clip_took > 0) also computes the group's clip -- from the SOURCE arrays, which nobody writes during the
// call, so no workgroup waits for another -- into n_clip[slot].  No atomics; the LDS is mask_clip_rule's.
__global__ __launch_bounds__(256) void group_gather_clip_kernel(const GroupGatherTable tab, int64_t words, int32_t n_chunks,
                                                                uint32_t *__restrict__ dst_bm, uint32_t *__restrict__ dst_chunks,
                                                                int64_t *__restrict__ n_clip)
{
    const int e = blockIdx.y;
    const uint32_t *__restrict__ src_bm = tab.bm[e];
    const uint32_t *__restrict__ src_ch = tab.chunks[e];
    const int64_t slot = tab.slot[e];
    const uint4 *__restrict__ in = reinterpret_cast<const uint4 *>(src_bm);
    uint4 *__restrict__ out = reinterpret_cast<uint4 *>(dst_bm + slot * words);
    const int64_t vecs = words >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < vecs; v += stride) out[v] = in[v];
    uint32_t *__restrict__ out_ch = dst_chunks + slot * (int64_t)n_chunks;      // (n_chunks need not be a multiple of 4: words of 4 bytes)
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += stride) out_ch[c] = src_ch[c];
    if (blockIdx.x != 0 || tab.clip_took[e] == 0u) return;
    mask_clip_rule(src_bm, words, n_chunks, src_ch, tab.clip_took[e], n_clip + slot);
}

hipError_t launch_group_gather_clip(const GroupGatherTable &tab, int32_t n_entries, int32_t n_slots, int64_t words, uint32_t *dst_bm,
                                    uint32_t *dst_chunks, int64_t *n_clip, hipStream_t s)
{
    if (n_entries <= 0) return hipSuccess;
    if (n_entries > kMaxGatherGroups || n_slots < 1 || n_slots > kMaxGatherGroups || words <= 0 || words % 4 != 0 || !dst_bm || !dst_chunks || !n_clip)
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(dst_bm) % 16 != 0) return hipErrorInvalidValue;
    for (int32_t e = 0; e < n_entries; ++e) {
        if (!tab.bm[e] || !tab.chunks[e] || reinterpret_cast<uintptr_t>(tab.bm[e]) % 16 != 0) return hipErrorInvalidValue;
        if (tab.slot[e] < 0 || tab.slot[e] >= n_slots) return hipErrorInvalidValue;
    }
    const int32_t n_chunks = scope_chunks(words);
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(((words >> 2) + 255) / 256, kGatherMaxBlocksX));
    hipLaunchKernelGGL(group_gather_clip_kernel, dim3(gx, (unsigned)n_entries), dim3(256), 0, s, tab, words, n_chunks, dst_bm, dst_chunks, n_clip);
    return hipGetLastError();
}

// launch_row_consts under a scope mask: a row whose bit is clear gets {0, mask::kMaskedRecency} -- no cosine part (x = 0 is the
// "normB <= 0" case of every screen) and a recency term below every floor a query can have.  The sentinel is finite:
// fused_epilogue16 turns non-finite row constants into "keep everything" and v_max3_f32 drops NaNs (orr_mask_plan.h has the
// bound); what reaches a buffer in spite of it is removed by mask_survivors.
__global__ __launch_bounds__(256) void row_consts_masked_kernel(const double *__restrict__ norm_b, const int64_t *__restrict__ created,
                                                                int64_t now_ticks, int64_t n_rows, const uint32_t *__restrict__ bitmap,
                                                                double2 *__restrict__ out)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
        double2 o;
        o.x = 0.0; o.y = mask::kMaskedRecency;
        if ((bitmap[r >> 5] >> (r & 31)) & 1u) o = row_consts_of(norm_b[r], created[r], now_ticks);
        out[r] = o;
    }
}

hipError_t launch_row_consts_masked(const double *norm_b, const int64_t *created, int64_t now_ticks, int64_t n_rows, const uint32_t *bitmap,
                                    double2 *out, hipStream_t s)
{
    if (n_rows <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n_rows + 255) / 256, 2048);
    hipLaunchKernelGGL(row_consts_masked_kernel, dim3((unsigned)blocks), dim3(256), 0, s, norm_b, created, now_ticks, n_rows, bitmap, out);
    return hipGetLastError();
}

// Behind the screen, one workgroup per query: buf[b][0 .. min(cnt, cap)) compacted in place, in order, to the entries
// mask::survivor_in_scope keeps.  Tiles of 256 entries: a tile is read before anything of it is written, and what a tile
// writes lies in front of the next tile.  cnt[b] becomes the kept count, except where the buffer had overflowed: that count
// stays (cnt > cap is the overflow signal of the tail's trailer, and the size the grown buffers are derived from).
__global__ __launch_bounds__(256) void mask_survivors_kernel(const uint32_t *__restrict__ bitmap, int64_t n_clip, uint32_t *__restrict__ cnt,
                                                             uint32_t cap, SelEntry *__restrict__ buf)
{
    __shared__ uint32_t wave_kept[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t c = cnt[b], n = c < cap ? c : cap;
    SelEntry *mine = buf + (int64_t)b * cap;
    uint32_t out = 0;
    for (uint32_t base = 0; base < n; base += 256u) {
        const uint32_t i = base + (uint32_t)tid;
        SelEntry e;
        e.key = 0ull; e.pos = 0u; e.pad = 0u;
        bool keep = false;
        if (i < n) {
            e = mine[i];
            keep = mask::survivor_in_scope(bitmap, e.pos, (uint64_t)n_clip);
        }
        const unsigned long long kept = __ballot(keep);
        const uint32_t rank = (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
        __syncthreads();                               // the tile is in registers; the last round's wave_kept has been read
        if (lane == 0) wave_kept[wave] = (uint32_t)__popcll(kept);
        __syncthreads();
        uint32_t at = out + rank;
        for (int k = 0; k < wave; ++k) at += wave_kept[k];
        if (keep) mine[at] = e;
        out += wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
    }
    if (tid == 0) cnt[b] = c > cap ? c : out;
}

hipError_t launch_mask_survivors(const uint32_t *bitmap, int64_t n_clip, uint32_t *cnt, uint32_t cap, SelEntry *buf, int32_t B, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    if (cap == 0u || n_clip < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_survivors_kernel, dim3((unsigned)B), dim3(256), 0, s, bitmap, n_clip, cnt, cap, buf);
    return hipGetLastError();
}

// One part of the list path: out = the set bits of `bitmap` whose rank lies in [first, last) (mask::part_word), every word of
// out written.  Workgroup per chunk, ranks as scope_compact_kernel forms them.
__global__ __launch_bounds__(256) void mask_part_kernel(const uint32_t *__restrict__ bitmap, int64_t words, const uint32_t *__restrict__ chunk_cnt,
                                                        uint64_t first, uint64_t last, uint32_t *__restrict__ out)
{
    __shared__ uint32_t sh4[4];
    __shared__ uint32_t wave_base[4];
    const int chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t before = 0;
    for (int c = tid; c < chunk; c += 256) before += chunk_cnt[c];
    before = block_sum_u32(before, sh4);
    const int64_t w0 = (int64_t)chunk * kScopeChunkWords + (int64_t)tid * 4;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (w0 < words) {
        const uint4 v = *reinterpret_cast<const uint4 *>(bitmap + w0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    const uint32_t own = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
    uint32_t incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wave_base[wave] = incl;
    __syncthreads();
    uint64_t rank = (uint64_t)before + incl - own;
    for (int k = 0; k < wave; ++k) rank += wave_base[k];
    if (w0 >= words) return;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[k] = mask::part_word(w[k], rank, first, last);
        rank += __popc(w[k]);
    }
    *reinterpret_cast<uint4 *>(out + w0) = make_uint4(o[0], o[1], o[2], o[3]);
}

hipError_t launch_mask_part(const uint32_t *bitmap, int64_t words, const uint32_t *chunk_cnt, uint64_t first, uint64_t last, uint32_t *out,
                            hipStream_t s)
{
    if (words <= 0 || words % 4 != 0 || last < first) return hipErrorInvalidValue;
    const int32_t n_chunks = scope_chunks(words);
    hipLaunchKernelGGL(mask_part_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, bitmap, words, chunk_cnt, first, last, out);
    return hipGetLastError();
}

// The trailers the two-stage tail wrote behind a masked screen: the floor stays (ORR_CAND_TWO_STAGE, L in norm_b); the rows
// that took part are the scope's first `took`.
__global__ void mask_trailers_kernel(orr_candidate *recs, int32_t B, int32_t kprime, int64_t took)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    recs[(int64_t)b * ((int64_t)kprime + 1) + kprime].order_key = took;
}

hipError_t launch_mask_trailers(orr_candidate *recs, int32_t B, int32_t kprime, int64_t took, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(mask_trailers_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, recs, B, kprime, took);
    return hipGetLastError();
}

// ---- grouped masked search (orr_search_batch_masked_groups; the rules are orr_group_plan.h's) ------------------------------

// launch_row_consts under G scope masks at once: a row keeps its real constants when some group holds it in front of that
// group's own clip (mask::survivor_in_scope per group: the 32 rows of a word read the same G words), else it gets the masked
// row's constants as row_consts_masked_kernel gives them.  A group with clip 0 takes no part.
__global__ __launch_bounds__(256) void row_consts_grouped_kernel(const double *__restrict__ norm_b, const int64_t *__restrict__ created,
                                                                 int64_t now_ticks, int64_t n_rows, const uint32_t *__restrict__ bitmaps,
                                                                 int64_t words, int32_t n_groups, const int64_t *__restrict__ clip,
                                                                 double2 *__restrict__ out)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
        bool held = false;
        for (int32_t g = 0; g < n_groups && !held; ++g)
            held = mask::survivor_in_scope(bitmaps + (int64_t)g * words, (uint32_t)r, (uint64_t)clip[g]);
        double2 o;
        o.x = 0.0; o.y = mask::kMaskedRecency;
        if (held) o = row_consts_of(norm_b[r], created[r], now_ticks);
        out[r] = o;
    }
}

hipError_t launch_row_consts_grouped(const double *norm_b, const int64_t *created, int64_t now_ticks, int64_t n_rows, const uint32_t *bitmaps,
                                     int64_t words, int32_t n_groups, const int64_t *clip, double2 *out, hipStream_t s)
{
    if (n_rows <= 0) return hipSuccess;
    if (n_groups <= 0 || words <= 0 || n_rows > words * 32) return hipErrorInvalidValue;      // (every row has its bit in every bitmap)
    const int64_t blocks = std::min<int64_t>((n_rows + 255) / 256, 2048);
    hipLaunchKernelGGL(row_consts_grouped_kernel, dim3((unsigned)blocks), dim3(256), 0, s, norm_b, created, now_ticks, n_rows, bitmaps, words,
                       n_groups, clip, out);
    return hipGetLastError();
}

// mask_survivors_kernel against the bitmap and the clip of the query's own group: a row of another group that beat this
// query's floor was buffered by the screen and goes here.  Tiles, order and the overflow signal as there.
__global__ __launch_bounds__(256) void mask_survivors_grouped_kernel(const uint32_t *__restrict__ bitmaps, int64_t words, int32_t n_groups,
                                                                     const int64_t *__restrict__ clip, const uint32_t *__restrict__ qgroup,
                                                                     uint32_t *__restrict__ cnt, uint32_t cap, SelEntry *__restrict__ buf)
{
    __shared__ uint32_t wave_kept[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = qgroup[b];
    const bool known = g < (uint32_t)n_groups;                     // (a query without a group keeps nothing)
    const uint32_t *bitmap = bitmaps + (int64_t)(known ? g : 0u) * words;
    const uint64_t n_clip = known && clip[g] > 0 ? (uint64_t)clip[g] : 0ull;
    const uint32_t c = cnt[b], n = c < cap ? c : cap;
    SelEntry *mine = buf + (int64_t)b * cap;
    uint32_t out = 0;
    for (uint32_t base = 0; base < n; base += 256u) {
        const uint32_t i = base + (uint32_t)tid;
        SelEntry e;
        e.key = 0ull; e.pos = 0u; e.pad = 0u;
        bool keep = false;
        if (i < n) {
            e = mine[i];
            keep = mask::survivor_in_scope(bitmap, e.pos, n_clip);
        }
        const unsigned long long kept = __ballot(keep);
        const uint32_t rank = (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
        __syncthreads();                               // the tile is in registers; the last round's wave_kept has been read
        if (lane == 0) wave_kept[wave] = (uint32_t)__popcll(kept);
        __syncthreads();
        uint32_t at = out + rank;
        for (int k = 0; k < wave; ++k) at += wave_kept[k];
        if (keep) mine[at] = e;
        out += wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
    }
    if (tid == 0) cnt[b] = c > cap ? c : out;
}

hipError_t launch_mask_survivors_grouped(const uint32_t *bitmaps, int64_t words, int32_t n_groups, const int64_t *clip, const uint32_t *qgroup,
                                         uint32_t *cnt, uint32_t cap, SelEntry *buf, int32_t B, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    if (cap == 0u || n_groups <= 0 || words <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_survivors_grouped_kernel, dim3((unsigned)B), dim3(256), 0, s, bitmaps, words, n_groups, clip, qgroup, cnt, cap, buf);
    return hipGetLastError();
}

// mask_trailers_kernel with the rows that took part per query: the first took[b] of its group's scope.
__global__ void mask_trailers_grouped_kernel(orr_candidate *recs, int32_t B, int32_t kprime, const int64_t *__restrict__ took)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    recs[(int64_t)b * ((int64_t)kprime + 1) + kprime].order_key = took[b];
}

hipError_t launch_mask_trailers_grouped(orr_candidate *recs, int32_t B, int32_t kprime, const int64_t *took, hipStream_t s)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(mask_trailers_grouped_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, recs, B, kprime, took);
    return hipGetLastError();
}

// ---- scope handles (orr_scope; the rules are orr_scope_set_plan.h's) ---------------------------------------------------------
// All of these stream a bitmap of a bit per row once: nothing next to a search.  They must be exact, not fast.

// bits [p0, p1) set, every other bit of the `words` words clear: four words per thread, every word written
__global__ __launch_bounds__(256) void scope_fill_range_kernel(uint32_t *__restrict__ bitmap, int64_t words, int64_t p0, int64_t p1)
{
    const int64_t w0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (w0 >= words) return;                           // (words is a multiple of 4: whole uint4s)
    *reinterpret_cast<uint4 *>(bitmap + w0) = make_uint4(scope_set::range_word(w0, p0, p1), scope_set::range_word(w0 + 1, p0, p1),
                                                         scope_set::range_word(w0 + 2, p0, p1), scope_set::range_word(w0 + 3, p0, p1));
}

hipError_t launch_scope_fill_range(uint32_t *bitmap, int64_t words, int64_t p0, int64_t p1, hipStream_t s)
{
    if (words <= 0 || words % 4 != 0 || p0 < 0 || p1 > words * 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_fill_range_kernel, dim3((unsigned)((words / 4 + 255) / 256)), dim3(256), 0, s, bitmap, words, p0, p1);
    return hipGetLastError();
}

// the bit of every listed position cleared (positions outside the bitmap are passed over)
__global__ __launch_bounds__(256) void scope_clear_positions_kernel(uint32_t *__restrict__ bitmap, int64_t words, const int64_t *__restrict__ pos,
                                                                    int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i];
    if (p < 0 || p >= words * 32) return;
    atomicAnd(bitmap + (p >> 5), ~(1u << (uint32_t)(p & 31)));
}

hipError_t launch_scope_clear_positions(uint32_t *bitmap, int64_t words, const int64_t *pos, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (words <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_clear_positions_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bitmap, words, pos, n);
    return hipGetLastError();
}

// dst = dst op src over 16-byte vectors, in place (scope_set::combine_word)
__global__ __launch_bounds__(256) void scope_combine_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, int64_t words, int32_t op)
{
    const int64_t w0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (w0 >= words) return;
    const uint4 a = *reinterpret_cast<const uint4 *>(dst + w0), b = *reinterpret_cast<const uint4 *>(src + w0);
    *reinterpret_cast<uint4 *>(dst + w0) = make_uint4(scope_set::combine_word(a.x, b.x, op), scope_set::combine_word(a.y, b.y, op),
                                                      scope_set::combine_word(a.z, b.z, op), scope_set::combine_word(a.w, b.w, op));
}

hipError_t launch_scope_combine(uint32_t *dst, const uint32_t *src, int64_t words, int32_t op, hipStream_t s)
{
    if (words <= 0 || words % 4 != 0 || !scope_set::op_valid(op)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_combine_kernel, dim3((unsigned)((words / 4 + 255) / 256)), dim3(256), 0, s, dst, src, words, op);
    return hipGetLastError();
}

// Carries n_scopes bitmaps through a move of rows (compaction, insertion).  One lane per destination row: its source position
// (scope_set::remap_source) is read ONCE, then for every scope the lane fetches its source bit and a ballot forms the wave's 64
// destination bits, which lane 0 stores as one 8-byte word pair.  Every word of the new bitmaps is written; rows at or above
// n_new and the padding words come out zero because remap_source gives them no source.  The sources of a wave are monotone and
// almost consecutive (rows keep their order), so its source bits lie in two or three words that come from cache.
__global__ __launch_bounds__(256) void scope_remap_kernel(const int64_t *__restrict__ src, int64_t first, int64_t n_new, int64_t new_words,
                                                          const uint32_t *const *__restrict__ old_bm, int64_t old_words,
                                                          uint32_t *const *__restrict__ new_bm, int32_t n_scopes)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t d0 = d & ~(int64_t)63;               // the wave's first row: 64 rows = two whole words
    if (d0 >= new_words * 32) return;                  // (wave-uniform; new_words is a multiple of 4)
    const int64_t sp = scope_set::remap_source(d, first, n_new, src);
    for (int32_t g = 0; g < n_scopes; ++g) {
        const unsigned long long bits = __ballot(scope_set::bit_at(old_bm[g], old_words, sp) != 0u);
        if ((threadIdx.x & 63) == 0) *reinterpret_cast<uint2 *>(new_bm[g] + (d0 >> 5)) = make_uint2((uint32_t)bits, (uint32_t)(bits >> 32));
    }
}

hipError_t launch_scope_remap(const int64_t *src, int64_t first, int64_t n_new, int64_t new_words, const uint32_t *const *old_bm,
                              int64_t old_words, uint32_t *const *new_bm, int32_t n_scopes, hipStream_t s)
{
    if (n_scopes <= 0) return hipSuccess;
    if (new_words <= 0 || new_words % 4 != 0 || old_words <= 0 || first < 0 || n_new < first || n_new > new_words * 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_remap_kernel, dim3((unsigned)((new_words * 32 + 255) / 256)), dim3(256), 0, s, src, first, n_new, new_words, old_bm,
                       old_words, new_bm, n_scopes);
    return hipGetLastError();
}

// out[i] = row_ids[buf[i].pos]: the ids of compacted scope entries, in candidate order
__global__ __launch_bounds__(256) void scope_entry_ids_kernel(const SelEntry *__restrict__ buf, int64_t n, const int64_t *__restrict__ row_ids,
                                                              int64_t n_rows, int64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = buf[i].pos;
    out[i] = (int64_t)p < n_rows ? row_ids[p] : -1;
}

hipError_t launch_scope_entry_ids(const SelEntry *buf, int64_t n, const int64_t *row_ids, int64_t n_rows, int64_t *out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scope_entry_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, buf, n, row_ids, n_rows, out);
    return hipGetLastError();
}

// ---- row keys and the per-key search (orr_keys, orr_search_batch_per_key; the rules are orr_per_key_plan.h's) -----------------

// the wave's OR of a 64-bit value, in every lane (a butterfly over the two halves)
__device__ __forceinline__ uint64_t wave_or_u64(uint64_t v)
{
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, off, 64);
        hi |= (uint32_t)__shfl_xor((int)hi, off, 64);
    }
    return ((uint64_t)hi << 32) | lo;
}

// A workgroup owns per_key::kBlockRows rows = kBlockWords words of every slot.  Each lane loads its eight keys (coalesced 8-byte
// loads) and searches the union table once per key (LDS: the table is staged first; otherwise it is read from global memory and
// stays in L2).  A workgroup none of whose rows is closed -- the common case: closed keys are a few thousand rows of millions --
// copies its base words into every slot as 16-byte vectors.  Any other workgroup builds the slots' words in an LDS tile: the
// tile starts as the base, then a wave with a closed row forms, for every slot in the OR of its lanes' masks, the slot's 64
// bits with one ballot (per_key::exclude_bits); the tile leaves as 16-byte vectors too.  Either way a slot receives
// 256 contiguous bytes per workgroup instead of 8 bytes per wave.  Every word of the n_slots bitmaps is written.  No atomics.
template <bool LDS>
__global__ __launch_bounds__(256) void keys_exclude_kernel(const int64_t *__restrict__ key, int64_t n_rows, const uint32_t *__restrict__ base,
                                                           int64_t words, const int64_t *__restrict__ tab_keys,
                                                           const uint64_t *__restrict__ tab_masks, int32_t n_tab, int32_t n_slots,
                                                           uint32_t *__restrict__ out)
{
    __shared__ int64_t sh_keys[LDS ? per_key::kLdsTable : 1];
    __shared__ uint64_t sh_masks[LDS ? per_key::kLdsTable : 1];
    __shared__ __attribute__((aligned(16))) uint32_t tile[per_key::kMaxSlots][per_key::kBlockWords];
    const int tid = threadIdx.x;
    if (LDS) {
        for (int i = tid; i < n_tab; i += 256) { sh_keys[i] = tab_keys[i]; sh_masks[i] = tab_masks[i]; }
        __syncthreads();
    }
    const int64_t *tk = LDS ? sh_keys : tab_keys;
    const uint64_t *tm = LDS ? sh_masks : tab_masks;
    const int64_t w0 = (int64_t)blockIdx.x * per_key::kBlockWords;
    if (w0 >= words) return;                           // (workgroup-uniform)
    const int wc = (int)(words - w0 < per_key::kBlockWords ? words - w0 : per_key::kBlockWords);      // a multiple of 4
    const int64_t row0 = w0 * 32;
    uint64_t m[8];
    int any = 0;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int64_t r = row0 + it * 256 + tid;
        const int64_t k = r < n_rows ? key[r] : per_key::kNone;
        m[it] = per_key::table_mask(tk, tm, n_tab, k);
        any |= m[it] != 0ull;
    }
    const int hit = __syncthreads_or(any);
    const int vec = wc >> 2;                           // 16-byte vectors per slot
    const uint4 *base4 = reinterpret_cast<const uint4 *>(base + w0);
    if (!hit) {
        for (int i = tid; i < n_slots * vec; i += 256) {
            const int s = i / vec, j = i - s * vec;
            reinterpret_cast<uint4 *>(out + (int64_t)s * words + w0)[j] = base4[j];
        }
        return;
    }
    for (int i = tid; i < n_slots * per_key::kBlockWords; i += 256) {
        const int s = i >> 6, j = i & 63;
        tile[s][j] = j < wc ? base[w0 + j] : 0u;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        uint64_t o = wave_or_u64(m[it]);               // the same in every lane of the wave
        const int wi = it * 8 + wave * 2;              // the wave's 64 rows: words wi, wi + 1 of the workgroup's
        if (o == 0ull || wi >= wc) continue;
        const uint64_t b = (uint64_t)base[w0 + wi] | ((uint64_t)base[w0 + wi + 1] << 32);
        while (o) {
            const int s = __ffsll((long long)o) - 1;
            o &= o - 1ull;
            const uint64_t closed = __ballot(per_key::slot_closed(m[it], s));
            if (lane == 0 && s < n_slots) {
                const uint64_t v = per_key::exclude_bits(b, closed);
                tile[s][wi] = (uint32_t)v;
                tile[s][wi + 1] = (uint32_t)(v >> 32);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n_slots * vec; i += 256) {
        const int s = i / vec, j = i - s * vec;
        reinterpret_cast<uint4 *>(out + (int64_t)s * words + w0)[j] = *reinterpret_cast<const uint4 *>(&tile[s][j * 4]);
    }
}

hipError_t launch_keys_exclude(const int64_t *key, int64_t n_rows, const uint32_t *base, int64_t words, const int64_t *tab_keys,
                               const uint64_t *tab_masks, int32_t n_tab, int32_t n_slots, uint32_t *out, hipStream_t s)
{
    if (n_slots <= 0) return hipSuccess;
    if (words <= 0 || words % 4 != 0 || n_rows < 0 || n_rows > words * 32 || n_slots > per_key::kMaxSlots || n_tab < 0 || !key || !base || !out ||
        (n_tab > 0 && (!tab_keys || !tab_masks)))
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(base) % 16 != 0 || reinterpret_cast<uintptr_t>(out) % 16 != 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((words + per_key::kBlockWords - 1) / per_key::kBlockWords);
    if (per_key::table_in_lds(n_tab))
        hipLaunchKernelGGL(keys_exclude_kernel<true>, dim3(blocks), dim3(256), 0, s, key, n_rows, base, words, tab_keys, tab_masks, n_tab, n_slots, out);
    else
        hipLaunchKernelGGL(keys_exclude_kernel<false>, dim3(blocks), dim3(256), 0, s, key, n_rows, base, words, tab_keys, tab_masks, n_tab, n_slots, out);
    return hipGetLastError();
}

// The sibling of keys_exclude with the opposite rule (orr_search_batch_routed; the rules are orr_routed_plan.h's): slot s's
// bitmap holds the rows of `base` whose key the slot routed to.  The same ownership, loads and table search.  A workgroup none of
// whose rows is routed -- by far the common case: a few documents out of millions of rows -- stores zeros into its words of
// every slot as 16-byte vectors and does not read the base at all.  Any other workgroup builds the slots' words in an LDS tile
// that starts as zero: a wave with a routed row forms, for every slot in the OR of its lanes' masks, the slot's 64 bits with one
// ballot and stores routed::include_bits(base word pair, ballot); the tile leaves as 16-byte vectors, 256 contiguous bytes per
// slot.  Every word of the n_slots bitmaps is written; rows at or above n_rows are clear (their key reads as kNone).  No atomics.
template <bool LDS>
__global__ __launch_bounds__(256) void routed_include_kernel(const int64_t *__restrict__ key, int64_t n_rows, const uint32_t *__restrict__ base,
                                                           int64_t words, const int64_t *__restrict__ tab_keys,
                                                           const uint64_t *__restrict__ tab_masks, int32_t n_tab, int32_t n_slots,
                                                           uint32_t *__restrict__ out)
{
    __shared__ int64_t sh_keys[LDS ? per_key::kLdsTable : 1];
    __shared__ uint64_t sh_masks[LDS ? per_key::kLdsTable : 1];
    __shared__ __attribute__((aligned(16))) uint32_t tile[per_key::kMaxSlots][per_key::kBlockWords];
    const int tid = threadIdx.x;
    if (LDS) {
        for (int i = tid; i < n_tab; i += 256) { sh_keys[i] = tab_keys[i]; sh_masks[i] = tab_masks[i]; }
        __syncthreads();
    }
    const int64_t *tk = LDS ? sh_keys : tab_keys;
    const uint64_t *tm = LDS ? sh_masks : tab_masks;
    const int64_t w0 = (int64_t)blockIdx.x * per_key::kBlockWords;
    if (w0 >= words) return;                           // (workgroup-uniform)
    const int wc = (int)(words - w0 < per_key::kBlockWords ? words - w0 : per_key::kBlockWords);      // a multiple of 4
    const int64_t row0 = w0 * 32;
    uint64_t m[8];
    int any = 0;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int64_t r = row0 + it * 256 + tid;
        const int64_t k = r < n_rows ? key[r] : per_key::kNone;
        m[it] = per_key::table_mask(tk, tm, n_tab, k);
        any |= m[it] != 0ull;
    }
    const int hit = __syncthreads_or(any);
    const int vec = wc >> 2;                           // 16-byte vectors per slot
    if (!hit) {
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        for (int i = tid; i < n_slots * vec; i += 256) {
            const int s = i / vec, j = i - s * vec;
            reinterpret_cast<uint4 *>(out + (int64_t)s * words + w0)[j] = zero;
        }
        return;
    }
    for (int i = tid; i < n_slots * per_key::kBlockWords; i += 256) tile[i >> 6][i & 63] = 0u;
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        uint64_t o = wave_or_u64(m[it]);               // the same in every lane of the wave
        const int wi = it * 8 + wave * 2;              // the wave's 64 rows: words wi, wi + 1 of the workgroup's
        if (o == 0ull || wi >= wc) continue;
        const uint64_t b = (uint64_t)base[w0 + wi] | ((uint64_t)base[w0 + wi + 1] << 32);
        while (o) {
            const int s = __ffsll((long long)o) - 1;
            o &= o - 1ull;
            const uint64_t in = __ballot(per_key::slot_closed(m[it], s));
            if (lane == 0 && s < n_slots) {
                const uint64_t v = routed::include_bits(b, in);
                tile[s][wi] = (uint32_t)v;
                tile[s][wi + 1] = (uint32_t)(v >> 32);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n_slots * vec; i += 256) {
        const int s = i / vec, j = i - s * vec;
        reinterpret_cast<uint4 *>(out + (int64_t)s * words + w0)[j] = *reinterpret_cast<const uint4 *>(&tile[s][j * 4]);
    }
}

hipError_t launch_keys_include(const int64_t *key, int64_t n_rows, const uint32_t *base, int64_t words, const int64_t *tab_keys,
                               const uint64_t *tab_masks, int32_t n_tab, int32_t n_slots, uint32_t *out, hipStream_t s)
{
    if (n_slots <= 0) return hipSuccess;
    if (words <= 0 || words % 4 != 0 || n_rows < 0 || n_rows > words * 32 || n_slots > per_key::kMaxSlots || n_tab < 0 || !key || !base || !out ||
        (n_tab > 0 && (!tab_keys || !tab_masks)))
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(base) % 16 != 0 || reinterpret_cast<uintptr_t>(out) % 16 != 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((words + per_key::kBlockWords - 1) / per_key::kBlockWords);
    if (per_key::table_in_lds(n_tab))
        hipLaunchKernelGGL(routed_include_kernel<true>, dim3(blocks), dim3(256), 0, s, key, n_rows, base, words, tab_keys, tab_masks, n_tab, n_slots, out);
    else
        hipLaunchKernelGGL(routed_include_kernel<false>, dim3(blocks), dim3(256), 0, s, key, n_rows, base, words, tab_keys, tab_masks, n_tab, n_slots, out);
    return hipGetLastError();
}

// scope_clear_positions with a slot: pair i clears bit pos[i] of bitmap slot[i] (pairs outside the bitmaps are passed over)
__global__ __launch_bounds__(256) void keys_clear_seen_kernel(uint32_t *__restrict__ bitmaps, int64_t words, int32_t n_slots,
                                                              const int32_t *__restrict__ slot, const int64_t *__restrict__ pos, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i];
    const int32_t sl = slot[i];
    if (p < 0 || p >= words * 32 || sl < 0 || sl >= n_slots) return;
    atomicAnd(bitmaps + (int64_t)sl * words + (p >> 5), ~(1u << (uint32_t)(p & 31)));
}

hipError_t launch_keys_clear_seen(uint32_t *bitmaps, int64_t words, int32_t n_slots, const int32_t *slot, const int64_t *pos, int64_t n,
                                  hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (words <= 0 || n_slots <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_clear_seen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bitmaps, words, n_slots, slot, pos, n);
    return hipGetLastError();
}

// One lane per row, the table search of keys_exclude with one slot and no base (per_key::table_find: ORR_KEY_NONE is a key like
// any other here); a ballot forms the wave's 64 bits, lane 0 stores them.  Every word is written; rows at or above n_rows are clear.
template <bool LDS>
__global__ __launch_bounds__(256) void keys_member_kernel(const int64_t *__restrict__ key, int64_t n_rows, const int64_t *__restrict__ tab_keys,
                                                          int32_t n_tab, uint32_t *__restrict__ bm, int64_t words)
{
    __shared__ int64_t sh_keys[LDS ? per_key::kLdsTable : 1];
    const int tid = threadIdx.x;
    if (LDS) {
        for (int i = tid; i < n_tab; i += 256) sh_keys[i] = tab_keys[i];
        __syncthreads();
    }
    const int64_t *tk = LDS ? sh_keys : tab_keys;
    const int64_t r = (int64_t)blockIdx.x * 256 + tid;
    const int64_t r0 = r & ~(int64_t)63;
    if (r0 >= words * 32) return;                      // (wave-uniform; words is a multiple of 4)
    const bool in = r < n_rows && per_key::table_find(tk, n_tab, key[r]) >= 0;
    const unsigned long long bits = __ballot(in);
    if ((tid & 63) == 0) *reinterpret_cast<uint2 *>(bm + (r0 >> 5)) = make_uint2((uint32_t)bits, (uint32_t)(bits >> 32));
}

hipError_t launch_keys_member(const int64_t *key, int64_t n_rows, const int64_t *tab_keys, int32_t n_tab, uint32_t *bm, int64_t words,
                              hipStream_t s)
{
    if (words <= 0 || words % 4 != 0 || n_rows < 0 || n_rows > words * 32 || n_tab < 0 || !key || !bm || (n_tab > 0 && !tab_keys))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((words * 32 + 255) / 256);
    if (per_key::table_in_lds(n_tab))
        hipLaunchKernelGGL(keys_member_kernel<true>, dim3(blocks), dim3(256), 0, s, key, n_rows, tab_keys, n_tab, bm, words);
    else
        hipLaunchKernelGGL(keys_member_kernel<false>, dim3(blocks), dim3(256), 0, s, key, n_rows, tab_keys, n_tab, bm, words);
    return hipGetLastError();
}

// whether position p is in dead[0 .. n_dead) (ascending)
__device__ __forceinline__ bool keys_row_dead(const int64_t *__restrict__ dead, int32_t n_dead, int64_t p)
{
    int32_t dl = 0, dh = n_dead;
    while (dl < dh) {
        const int32_t mid = (dl + dh) >> 1;
        if (dead[mid] < p) dl = mid + 1; else dh = mid;
    }
    return dl < n_dead && dead[dl] == p;
}

// the position of the first live row that carries id `want` (scope_lookup's search over the id table), -1 when there is none
__device__ __forceinline__ int64_t first_live_row(const int64_t *__restrict__ table_ids, const uint32_t *__restrict__ table_pos, int64_t n_rows,
                                                  const int64_t *__restrict__ dead, int32_t n_dead, int64_t want)
{
    int64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (table_ids[mid] < want) lo = mid + 1; else hi = mid;
    }
    for (; lo < n_rows && table_ids[lo] == want; ++lo)
        if (!keys_row_dead(dead, n_dead, (int64_t)table_pos[lo])) return (int64_t)table_pos[lo];
    return -1;
}

__global__ __launch_bounds__(256) void keys_gather_kernel(const int64_t *__restrict__ key, int64_t n_rows, const int64_t *__restrict__ pos, int64_t n,
                                                          const int64_t *__restrict__ table_ids, const uint32_t *__restrict__ table_pos,
                                                          const int64_t *__restrict__ dead, int32_t n_dead, int64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t p = pos[i];
    if (table_ids) p = first_live_row(table_ids, table_pos, n_rows, dead, n_dead, p);   // pos[i] is a row id
    out[i] = (p >= 0 && p < n_rows) ? key[p] : per_key::kNone;
}

// orr_index_get_rows: out_pos[i] = the position of the first live row that carries id ids[i] (first_live_row: orr_keys_get's
// lookup), found[i] = 1; an unknown or deleted id: kRowsFindNone (at or above every n_rows: rows_gather writes zeros for it and
// reads nothing) and found[i] = 0.
__global__ __launch_bounds__(256) void rows_find_kernel(const int64_t *__restrict__ table_ids, const uint32_t *__restrict__ table_pos, int64_t n_rows,
                                                        const int64_t *__restrict__ ids, int64_t n, const int64_t *__restrict__ dead, int32_t n_dead,
                                                        uint32_t *__restrict__ out_pos, uint8_t *__restrict__ found)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t p = first_live_row(table_ids, table_pos, n_rows, dead, n_dead, ids[i]);
    out_pos[i] = p >= 0 ? (uint32_t)p : kRowsFindNone;
    found[i] = p >= 0 ? 1 : 0;
}

hipError_t launch_rows_find(const int64_t *table_ids, const uint32_t *table_pos, int64_t n_rows, const int64_t *ids, int64_t n, const int64_t *dead,
                            int32_t n_dead, uint32_t *out_pos, uint8_t *found, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (!table_ids || !table_pos || !ids || !out_pos || !found || n_rows < 0 || n_rows >= (int64_t)kRowsFindNone || (n_dead > 0 && !dead))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rows_find_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, table_ids, table_pos, n_rows, ids, n, dead, n_dead, out_pos,
                       found);
    return hipGetLastError();
}

hipError_t launch_keys_gather(const int64_t *key, int64_t n_rows, const int64_t *pos, int64_t n, const int64_t *table_ids,
                              const uint32_t *table_pos, const int64_t *dead, int32_t n_dead, int64_t *out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (!key || !pos || !out || n_rows < 0 || (table_ids && !table_pos) || (n_dead > 0 && !dead)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, key, n_rows, pos, n, table_ids, table_pos, dead,
                       n_dead, out);
    return hipGetLastError();
}

// One thread per entry: the run of equal ids in the table, every live position of it takes the entry's key.
__global__ __launch_bounds__(256) void keys_scatter_kernel(const int64_t *__restrict__ table_ids, const uint32_t *__restrict__ table_pos,
                                                           int64_t n_rows, const int64_t *__restrict__ ids, const int64_t *__restrict__ keys,
                                                           int64_t n, const int64_t *__restrict__ dead, int32_t n_dead,
                                                           int64_t *__restrict__ key, unsigned long long *__restrict__ n_set)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t want = ids[i];
    int64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (table_ids[mid] < want) lo = mid + 1; else hi = mid;
    }
    bool named = false;
    for (; lo < n_rows && table_ids[lo] == want; ++lo) {
        const int64_t p = (int64_t)table_pos[lo];
        if (p >= n_rows || keys_row_dead(dead, n_dead, p)) continue;
        key[p] = keys[i];
        named = true;
    }
    if (named) atomicAdd(n_set, 1ull);
}

hipError_t launch_keys_scatter(const int64_t *table_ids, const uint32_t *table_pos, int64_t n_rows, const int64_t *ids, const int64_t *keys,
                               int64_t n, const int64_t *dead, int32_t n_dead, int64_t *key, unsigned long long *n_set, hipStream_t s)
{
    if (n <= 0 || n_rows <= 0) return hipSuccess;
    if (!table_ids || !table_pos || !ids || !keys || !key || !n_set || (n_dead > 0 && !dead)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, table_ids, table_pos, n_rows, ids, keys, n, dead,
                       n_dead, key, n_set);
    return hipGetLastError();
}

// One lane per destination row, its source read ONCE (scope_set::remap_source, as scope_remap), then every column's key.
__global__ __launch_bounds__(256) void keys_remap_kernel(const int64_t *__restrict__ src, int64_t first, int64_t n_new,
                                                         const int64_t *const *__restrict__ old_key, int64_t *const *__restrict__ new_key,
                                                         int32_t n_cols)
{
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n_new) return;
    const int64_t sp = scope_set::remap_source(d, first, n_new, src);
    for (int32_t g = 0; g < n_cols; ++g) new_key[g][d] = sp >= 0 ? old_key[g][sp] : per_key::kNone;
}

hipError_t launch_keys_remap(const int64_t *src, int64_t first, int64_t n_new, const int64_t *const *old_key, int64_t *const *new_key,
                             int32_t n_cols, hipStream_t s)
{
    if (n_cols <= 0 || n_new <= 0) return hipSuccess;
    if (first < 0 || n_new < first || !old_key || !new_key || (n_new > first && !src)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_remap_kernel, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, s, src, first, n_new, old_key, new_key, n_cols);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void keys_fill_none_kernel(int64_t *__restrict__ key, int64_t n)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) key[r] = per_key::kNone;
}

hipError_t launch_keys_fill_none(int64_t *key, int64_t n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(keys_fill_none_kernel, dim3(capped_blocks(n, 256)), dim3(256), 0, s, key, n);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void keys_count_kernel(const int64_t *__restrict__ key, int64_t n_rows, const int64_t *__restrict__ dead,
                                                         int32_t n_dead, unsigned long long *__restrict__ out)
{
    unsigned long long c = 0;                          // one ballot per 64 rows, counted by lane 0 of the wave
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); r0 < n_rows; r0 += stride) {
        const int64_t r = r0 + (threadIdx.x & 63);
        const bool has = r < n_rows && key[r] != per_key::kNone && !keys_row_dead(dead, n_dead, r);
        c += (unsigned long long)__popcll(__ballot(has));
    }
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

hipError_t launch_keys_count(const int64_t *key, int64_t n_rows, const int64_t *dead, int32_t n_dead, unsigned long long *out, hipStream_t s)
{
    if (n_rows <= 0) return hipSuccess;
    if (!key || !out || (n_dead > 0 && !dead)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keys_count_kernel, dim3(capped_blocks(n_rows, 256)), dim3(256), 0, s, key, n_rows, dead, n_dead, out);
    return hipGetLastError();
}

// ---- key groups (orr_keys_groups, orr_keys_centroids, orr_scope_centroid; the rules are orr_key_groups_plan.h's) ---------------
// (The kernel functions are named key_groups_*: the keys_* kernels stay the key column's own.  Their launches appear in the
// kernel statistics as keys_pairs_count, keys_pairs, keys_block_sums and keys_block_fold.)

// One lane per row, two passes over the same selection.  A row is selected when its bit in bm is set (the live rows, or the
// call's scope) and, by MODE, 0: it has a key (orr_keys_groups; the pair's key is key_groups::sort_key), 1: its norm participates
// and its key is in the call's table (per_key::table_find, LDS or global as keys_member; the pair's key is the table index),
// 2: its norm participates (orr_scope_centroid; positions only), 3: its norm participates and it has a key
// (orr_keys_centroid_index; the pair's key is key_groups::sort_key).  The count pass (WRITE false) leaves the workgroup's selected
// rows in counts[blockIdx.x]; behind an exclusive scan of those the write pass compacts the pairs with the order kept: the
// workgroup's offset, the waves in front (LDS), the lanes in front (ballot and prefix).  No atomics decide an order.
template <int MODE, bool LDS, bool WRITE>
__global__ __launch_bounds__(256) void key_groups_pairs_kernel(const int64_t *__restrict__ key, const double *__restrict__ norm_b, int64_t n_rows,
                                                         const uint32_t *__restrict__ bm, const int64_t *__restrict__ tab_keys, int32_t n_tab,
                                                         uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets, int64_t cap,
                                                         uint64_t *__restrict__ out_key, uint32_t *__restrict__ out_pos)
{
    __shared__ int64_t sh_keys[(MODE == 1 && LDS) ? per_key::kLdsTable : 1];
    __shared__ uint32_t wave_cnt[4];
    const int tid = threadIdx.x;
    if (MODE == 1 && LDS) {
        for (int i = tid; i < n_tab; i += 256) sh_keys[i] = tab_keys[i];
        __syncthreads();
    }
    const int64_t *tk = (MODE == 1 && LDS) ? sh_keys : tab_keys;
    const int64_t r = (int64_t)blockIdx.x * 256 + tid;
    bool sel = false;
    uint64_t sk = 0;
    if (r < n_rows && ((bm[r >> 5] >> (uint32_t)(r & 31)) & 1u)) {
        if (MODE == 0) {
            const int64_t k = key[r];
            sel = k != per_key::kNone;
            sk = key_groups::sort_key(k);
        } else if (MODE == 1) {
            if (key_groups::participates(norm_b[r])) {
                const int32_t i = per_key::table_find(tk, n_tab, key[r]);
                sel = i >= 0;
                sk = (uint64_t)(uint32_t)i;
            }
        } else if (MODE == 3) {
            if (key_groups::participates(norm_b[r])) {
                const int64_t k = key[r];
                sel = k != per_key::kNone;
                sk = key_groups::sort_key(k);
            }
        } else {
            sel = key_groups::participates(norm_b[r]);
        }
    }
    const unsigned long long bits = __ballot(sel);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bits);
    __syncthreads();
    if (!WRITE) {
        if (tid == 0) counts[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        return;
    }
    int64_t at = offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) at += wave_cnt[w];
    at += __popcll(bits & ((1ull << lane) - 1ull));
    if (sel && at < cap) {
        if (MODE != 2) out_key[at] = sk;
        out_pos[at] = (uint32_t)r;
    }
}

template <int MODE, bool LDS>
static hipError_t launch_keys_pairs_form(bool write, unsigned blocks, hipStream_t s, const int64_t *key, const double *norm_b, int64_t n_rows,
                                         const uint32_t *bm, const int64_t *tab_keys, int32_t n_tab, uint32_t *counts, const uint32_t *offsets,
                                         int64_t cap, uint64_t *out_key, uint32_t *out_pos)
{
    if (write)
        hipLaunchKernelGGL((key_groups_pairs_kernel<MODE, LDS, true>), dim3(blocks), dim3(256), 0, s, key, norm_b, n_rows, bm, tab_keys, n_tab, counts,
                           offsets, cap, out_key, out_pos);
    else
        hipLaunchKernelGGL((key_groups_pairs_kernel<MODE, LDS, false>), dim3(blocks), dim3(256), 0, s, key, norm_b, n_rows, bm, tab_keys, n_tab, counts,
                           offsets, cap, out_key, out_pos);
    return hipGetLastError();
}

hipError_t launch_keys_pairs(int32_t mode, bool write, const int64_t *key, const double *norm_b, int64_t n_rows, const uint32_t *bm, int64_t words,
                             const int64_t *tab_keys, int32_t n_tab, uint32_t *counts, const uint32_t *offsets, int64_t cap, uint64_t *out_key,
                             uint32_t *out_pos, hipStream_t s)
{
    if (n_rows <= 0) return hipSuccess;
    if (mode < 0 || mode > 3 || !bm || n_rows > words * 32 || n_rows > (int64_t)0xFFFFFFFFll || (mode != 2 && !key) || (mode != 0 && !norm_b) ||
        (mode == 1 && (n_tab <= 0 || !tab_keys)) || (!write && !counts) || (write && (!offsets || !out_pos || cap <= 0 || (mode != 2 && !out_key))))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)key_groups_pair_blocks(n_rows);
    if (mode == 0) return launch_keys_pairs_form<0, false>(write, blocks, s, key, norm_b, n_rows, bm, tab_keys, n_tab, counts, offsets, cap, out_key, out_pos);
    if (mode == 2) return launch_keys_pairs_form<2, false>(write, blocks, s, key, norm_b, n_rows, bm, tab_keys, n_tab, counts, offsets, cap, out_key, out_pos);
    if (mode == 3) return launch_keys_pairs_form<3, false>(write, blocks, s, key, norm_b, n_rows, bm, tab_keys, n_tab, counts, offsets, cap, out_key, out_pos);
    if (per_key::table_in_lds(n_tab))
        return launch_keys_pairs_form<1, true>(write, blocks, s, key, norm_b, n_rows, bm, tab_keys, n_tab, counts, offsets, cap, out_key, out_pos);
    return launch_keys_pairs_form<1, false>(write, blocks, s, key, norm_b, n_rows, bm, tab_keys, n_tab, counts, offsets, cap, out_key, out_pos);
}

hipError_t keys_pairs_scan(void *temp, size_t &temp_bytes, const uint32_t *counts, uint32_t *offsets, int64_t n, hipStream_t s)
{
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, counts, offsets, (int)n, s);
}

hipError_t keys_pairs_sort(void *temp, size_t &temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *pos_in, uint32_t *pos_out,
                           int64_t n, int32_t end_bit, hipStream_t s)
{
    // (a stable radix sort: equal keys keep their positions ascending)
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, key_in, key_out, pos_in, pos_out, (int)n, 0, end_bit, s);
}

hipError_t keys_pairs_runs(void *temp, size_t &temp_bytes, const uint64_t *key_sorted, uint64_t *run_key, uint32_t *run_len, uint32_t *n_runs,
                           int64_t n, hipStream_t s)
{
    return hipcub::DeviceRunLengthEncode::Encode(temp, temp_bytes, key_sorted, run_key, run_len, n_runs, (int)n, s);
}

// The hot path: one workgroup per block of at most key_groups::kBlock participating members.  The block's positions are staged
// in LDS; a lane owns four consecutive coordinates per 1,024 (one 16-byte load per row where dim % 4 == 0, four guarded 4-byte
// loads otherwise), so a wave reads 1 KB of a row at a time, fully coalesced.  Eight rows' loads are issued before the first is
// used; the fp64 adds are taken strictly in member order, from +0.0 (key_groups::sum_blocked's P_j).  A key of one block writes
// its row of the sums, any other block its row of the partials.
template <bool VEC>
__global__ __launch_bounds__(256) void key_groups_block_sums_kernel(const float *__restrict__ emb, int32_t dim, const uint32_t *__restrict__ pos,
                                                              const key_groups::Block *__restrict__ blocks, double *__restrict__ sums,
                                                              double *__restrict__ parts)
{
    __shared__ uint32_t sh_pos[key_groups::kBlock];
    const key_groups::Block b = blocks[blockIdx.x];
    const int tid = threadIdx.x;
    if ((uint32_t)tid < b.len) sh_pos[tid] = pos[(size_t)b.first + tid];
    __syncthreads();
    double *out = b.part == key_groups::kDirect ? sums + (size_t)b.slot * dim : parts + (size_t)b.part * dim;
    for (int32_t d0 = tid * key_groups::kCoordsPerLane; d0 < dim; d0 += key_groups::kCoordsPerPass) {
        double a0 = +0.0, a1 = +0.0, a2 = +0.0, a3 = +0.0;
        const bool in1 = d0 + 1 < dim, in2 = d0 + 2 < dim, in3 = d0 + 3 < dim;
        auto load = [&](uint32_t i) -> float4 {
            const float *row = emb + (size_t)sh_pos[i] * dim + d0;
            if (VEC) return *reinterpret_cast<const float4 *>(row);
            return make_float4(row[0], in1 ? row[1] : 0.f, in2 ? row[2] : 0.f, in3 ? row[3] : 0.f);
        };
        uint32_t i = 0;
        for (; i + 8 <= b.len; i += 8) {
            float4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = load(i + j);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a0 = a0 + (double)v[j].x; a1 = a1 + (double)v[j].y; a2 = a2 + (double)v[j].z; a3 = a3 + (double)v[j].w;
            }
        }
        for (; i < b.len; ++i) {
            const float4 v = load(i);
            a0 = a0 + (double)v.x; a1 = a1 + (double)v.y; a2 = a2 + (double)v.z; a3 = a3 + (double)v.w;
        }
        if (VEC) {
            *reinterpret_cast<double2 *>(out + d0) = make_double2(a0, a1);
            *reinterpret_cast<double2 *>(out + d0 + 2) = make_double2(a2, a3);
        } else {
            out[d0] = a0;
            if (in1) out[d0 + 1] = a1;
            if (in2) out[d0 + 2] = a2;
            if (in3) out[d0 + 3] = a3;
        }
    }
}

hipError_t launch_keys_block_sums(const float *emb, int64_t n_rows, int32_t dim, const uint32_t *pos, const key_groups::Block *blocks,
                                  int64_t n_blocks, double *sums, double *parts, hipStream_t s)
{
    if (n_blocks <= 0) return hipSuccess;
    if (!emb || n_rows <= 0 || dim <= 0 || !pos || !blocks || !sums || n_blocks > (int64_t)0x7FFFFFFF) return hipErrorInvalidValue;
    const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(emb) % 16 == 0 && reinterpret_cast<uintptr_t>(sums) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(parts) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(key_groups_block_sums_kernel<true>, dim3((unsigned)n_blocks), dim3(256), 0, s, emb, dim, pos, blocks, sums, parts);
    else
        hipLaunchKernelGGL(key_groups_block_sums_kernel<false>, dim3((unsigned)n_blocks), dim3(256), 0, s, emb, dim, pos, blocks, sums, parts);
    return hipGetLastError();
}

// A key of several blocks: one thread per coordinate adds its partial rows in block order, from +0.0 (key_groups::sum_blocked's
// S); eight rows' loads are issued before the first is used.
__global__ __launch_bounds__(256) void key_groups_block_fold_kernel(const key_groups::Fold *__restrict__ folds, const double *__restrict__ parts,
                                                              int32_t dim, double *__restrict__ sums)
{
    const key_groups::Fold f = folds[blockIdx.x];
    const int32_t d = (int32_t)blockIdx.y * 256 + threadIdx.x;
    if (d >= dim) return;
    const double *p = parts + (size_t)f.part0 * dim + d;
    double s = +0.0;
    uint32_t b = 0;
    for (; b + 8 <= f.n_blocks; b += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(b + j) * dim];
#pragma unroll
        for (int j = 0; j < 8; ++j) s = s + v[j];
    }
    for (; b < f.n_blocks; ++b) s = s + p[(size_t)b * dim];
    sums[(size_t)f.slot * dim + d] = s;
}

hipError_t launch_keys_block_fold(const key_groups::Fold *folds, int64_t n_folds, const double *parts, int32_t dim, double *sums, hipStream_t s)
{
    if (n_folds <= 0) return hipSuccess;
    if (!folds || !parts || !sums || dim <= 0 || n_folds > (int64_t)0x7FFFFFFF || (dim + 255) / 256 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(key_groups_block_fold_kernel, dim3((unsigned)n_folds, (unsigned)((dim + 255) / 256)), dim3(256), 0, s, folds, parts, dim, sums);
    return hipGetLastError();
}

// ---- the document index (orr_keys_centroid_index; the rules are orr_centroid_index_plan.h's) ----------------------------------
// keys_centroid_finish: a streaming kernel, one lane per kept key and four consecutive coordinates (two 16-byte loads of the
// key's fp64 sums, one 16-byte store of its fp32 centroid where VEC; guarded 8-byte loads and 4-byte stores otherwise).  Lanes
// run along a key's coordinates first, so a wave reads 2 KB of sums and writes 1 KB of centroids, both contiguous.  The
// expression is key_groups::finish_one, the host's.  The lane of a key's first coordinates also gathers the key's ticks
// (keys_first_ticks, folded into this launch): created[pos[first]], its first participating member's.  No LDS, no atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void key_groups_centroid_finish_kernel(const double *__restrict__ sums, int32_t dim, int32_t quads,
                                                                   const centroid_index::Kept *__restrict__ kept, int64_t n_kept,
                                                                   const uint32_t *__restrict__ pos, const int64_t *__restrict__ created,
                                                                   float *__restrict__ out, int64_t *__restrict__ out_ticks)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t / quads;
    if (i >= n_kept) return;
    const int32_t d0 = (int32_t)(t - i * quads) * 4;
    const centroid_index::Kept k = kept[i];
    if (d0 == 0) out_ticks[i] = created[pos[k.first]];
    const double *S = sums + (size_t)k.slot * dim + d0;
    float *c = out + (size_t)i * dim + d0;
    const int64_t n = (int64_t)k.n;
    if (VEC) {
        const double2 a = *reinterpret_cast<const double2 *>(S), b = *reinterpret_cast<const double2 *>(S + 2);
        *reinterpret_cast<float4 *>(c) = make_float4(key_groups::finish_one(a.x, n), key_groups::finish_one(a.y, n), key_groups::finish_one(b.x, n),
                                                     key_groups::finish_one(b.y, n));
    } else {
        for (int32_t j = 0; j < 4 && d0 + j < dim; ++j) c[j] = key_groups::finish_one(S[j], n);
    }
}

hipError_t launch_keys_centroid_finish(const double *sums, int32_t dim, const centroid_index::Kept *kept, int64_t n_kept, const uint32_t *pos,
                                       const int64_t *created, float *out, int64_t *out_ticks, hipStream_t s)
{
    if (n_kept <= 0) return hipSuccess;
    if (!sums || dim <= 0 || !kept || !pos || !created || !out || !out_ticks) return hipErrorInvalidValue;
    const int32_t quads = (dim + 3) / 4;
    const int64_t blocks = (n_kept * quads + 255) / 256;
    if (blocks > (int64_t)0x7FFFFFFF) return hipErrorInvalidValue;
    const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(sums) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(key_groups_centroid_finish_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, sums, dim, quads, kept, n_kept, pos, created,
                           out, out_ticks);
    else
        hipLaunchKernelGGL(key_groups_centroid_finish_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, sums, dim, quads, kept, n_kept, pos,
                           created, out, out_ticks);
    return hipGetLastError();
}

// ---- cluster key groups (orr_cluster_keys_centroids, orr_cluster_scope_centroid; the rules are orr_cluster_key_groups_plan.h's) --
// keys_chain_step: one shard's step of the keys that span shards.  One workgroup per Chain record and 1,024 coordinates, the lane
// layout of keys_block_sums (a lane owns four consecutive coordinates; one 16-byte load per head row where VEC).  Per coordinate,
// strictly in this order, all fp64: P from the carried P row (or +0.0) over the head fragment in member order; S from the carried S
// row (or +0.0), plus P where the head's block closes here, plus the partial rows of the free blocks that close here in block order
// (double2 loads, eight ahead, as keys_block_fold); S and the open block's partial go to the key's state rows.
template <bool VEC>
__global__ __launch_bounds__(256) void key_groups_chain_kernel(const float *__restrict__ emb, int32_t dim, const uint32_t *__restrict__ pos,
                                                         const cluster_key_groups::Chain *__restrict__ chains,
                                                         const double *__restrict__ parts, double *__restrict__ state)
{
    __shared__ uint32_t sh_pos[key_groups::kBlock];
    const cluster_key_groups::Chain c = chains[blockIdx.x];
    const int tid = threadIdx.x;
    if ((uint32_t)tid < c.head_len) sh_pos[tid] = pos[(size_t)c.head_first + tid];
    __syncthreads();
    const int32_t d0 = (int32_t)blockIdx.y * key_groups::kCoordsPerPass + tid * key_groups::kCoordsPerLane;
    if (d0 >= dim) return;
    const bool in1 = d0 + 1 < dim, in2 = d0 + 2 < dim, in3 = d0 + 3 < dim;
    double *s_row = state + (size_t)c.state * 2 * dim + d0, *p_row = s_row + dim;
    auto load_row = [&](const double *row, double &x0, double &x1, double &x2, double &x3) {
        if (VEC) {
            const double2 lo = *reinterpret_cast<const double2 *>(row), hi = *reinterpret_cast<const double2 *>(row + 2);
            x0 = lo.x; x1 = lo.y; x2 = hi.x; x3 = hi.y;
        } else {
            x0 = row[0]; x1 = in1 ? row[1] : +0.0; x2 = in2 ? row[2] : +0.0; x3 = in3 ? row[3] : +0.0;
        }
    };
    auto store_row = [&](double *row, double x0, double x1, double x2, double x3) {
        if (VEC) {
            *reinterpret_cast<double2 *>(row) = make_double2(x0, x1);
            *reinterpret_cast<double2 *>(row + 2) = make_double2(x2, x3);
        } else {
            row[0] = x0;
            if (in1) row[1] = x1;
            if (in2) row[2] = x2;
            if (in3) row[3] = x3;
        }
    };
    // 1, 2: the head fragment continues the open block
    double p0 = +0.0, p1 = +0.0, p2 = +0.0, p3 = +0.0;
    if (cluster_key_groups::chain_seed_p(c.flags)) load_row(p_row, p0, p1, p2, p3);
    auto load = [&](uint32_t i) -> float4 {
        const float *row = emb + (size_t)sh_pos[i] * dim + d0;
        if (VEC) return *reinterpret_cast<const float4 *>(row);
        return make_float4(row[0], in1 ? row[1] : 0.f, in2 ? row[2] : 0.f, in3 ? row[3] : 0.f);
    };
    uint32_t i = 0;
    for (; i + 8 <= c.head_len; i += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = load(i + j);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            p0 = p0 + (double)v[j].x; p1 = p1 + (double)v[j].y; p2 = p2 + (double)v[j].z; p3 = p3 + (double)v[j].w;
        }
    }
    for (; i < c.head_len; ++i) {
        const float4 v = load(i);
        p0 = p0 + (double)v.x; p1 = p1 + (double)v.y; p2 = p2 + (double)v.z; p3 = p3 + (double)v.w;
    }
    // 3: the running sum, and the head's block where it closes here
    double s0 = +0.0, s1 = +0.0, s2 = +0.0, s3 = +0.0;
    if (cluster_key_groups::chain_seed_s(c.flags)) load_row(s_row, s0, s1, s2, s3);
    if (cluster_key_groups::chain_head_closes(c.flags)) {
        s0 = s0 + p0; s1 = s1 + p1; s2 = s2 + p2; s3 = s3 + p3;
    }
    // 4: the free blocks that close here, in block order
    const double *q = parts + (size_t)c.part0 * dim + d0;
    uint32_t b = 0;
    for (; b + 8 <= c.n_close; b += 8) {
        double w[8][4];
#pragma unroll
        for (int j = 0; j < 8; ++j) load_row(q + (size_t)(b + j) * dim, w[j][0], w[j][1], w[j][2], w[j][3]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s0 = s0 + w[j][0]; s1 = s1 + w[j][1]; s2 = s2 + w[j][2]; s3 = s3 + w[j][3];
        }
    }
    for (; b < c.n_close; ++b) {
        double w0, w1, w2, w3;
        load_row(q + (size_t)b * dim, w0, w1, w2, w3);
        s0 = s0 + w0; s1 = s1 + w1; s2 = s2 + w2; s3 = s3 + w3;
    }
    // 5: the state the next shard with a member continues from
    store_row(s_row, s0, s1, s2, s3);
    const uint32_t open = cluster_key_groups::chain_open(c.flags);
    if (open == cluster_key_groups::kOpenHead) {
        store_row(p_row, p0, p1, p2, p3);
    } else if (open == cluster_key_groups::kOpenFree) {
        double w0, w1, w2, w3;
        load_row(q + (size_t)c.n_close * dim, w0, w1, w2, w3);
        store_row(p_row, w0, w1, w2, w3);
    }
}

hipError_t launch_keys_chain_step(const float *emb, int64_t n_rows, int32_t dim, const uint32_t *pos, const cluster_key_groups::Chain *chains,
                                  int64_t n_chains, const double *parts, double *state, hipStream_t s)
{
    if (n_chains <= 0) return hipSuccess;
    const int64_t tiles = ((int64_t)dim + key_groups::kCoordsPerPass - 1) / key_groups::kCoordsPerPass;
    if (!emb || n_rows <= 0 || dim <= 0 || !pos || !chains || !state || n_chains > (int64_t)0x7FFFFFFF || tiles > 65535) return hipErrorInvalidValue;
    const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(emb) % 16 == 0 && reinterpret_cast<uintptr_t>(state) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(parts) % 16 == 0;
    const dim3 grid((unsigned)n_chains, (unsigned)tiles);
    if (vec)
        hipLaunchKernelGGL(key_groups_chain_kernel<true>, grid, dim3(256), 0, s, emb, dim, pos, chains, parts, state);
    else
        hipLaunchKernelGGL(key_groups_chain_kernel<false>, grid, dim3(256), 0, s, emb, dim, pos, chains, parts, state);
    return hipGetLastError();
}

// ---- term scopes (orr_scope_create_terms; the rules are orr_scope_terms_plan.h's) -------------------------------------------

// where each distinct term's bitmap starts (n <= 256 values: one workgroup)
__global__ __launch_bounds__(256) void scope_terms_bases_kernel(const int64_t *__restrict__ term_word_off, int32_t n, int64_t words,
                                                                int64_t *__restrict__ term_base, int64_t *__restrict__ term_base_host)
{
    const int32_t t = threadIdx.x;
    if (t >= n) return;
    const int64_t base = term_word_off ? term_word_off[t] : (int64_t)t * words;
    term_base[t] = base;
    if (term_base_host) term_base_host[t] = base;
}

hipError_t launch_scope_terms_bases(const int64_t *term_word_off, int32_t n, int64_t words, int64_t *term_base, int64_t *term_base_host,
                                    hipStream_t s)
{
    if (n < 1 || n > scope_terms::kMaxTerms || words <= 0 || !term_base) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_terms_bases_kernel, dim3(1), dim3(256), 0, s, term_word_off, n, words, term_base, term_base_host);
    return hipGetLastError();
}

// One lane per 16-byte vector of dst, grid-stride: the lane loads the same vector of each term's bitmap (consecutive lanes,
// consecutive vectors: every load of a wave is one contiguous 1 KiB), folds them (scope_terms::fold_word), masks the tail
// (scope_terms::tail_mask) and stores once.  The bases are the same for every lane: they come through the scalar cache.
__global__ __launch_bounds__(256) void scope_terms_combine_kernel(const uint32_t *__restrict__ bitmaps, const int64_t *__restrict__ term_base,
                                                                  int32_t n, int32_t mode, int64_t words, int64_t n_rows, uint32_t *__restrict__ dst)
{
    const int64_t n_vec = words / 4, stride = (int64_t)gridDim.x * 256;
    const uint32_t id = scope_terms::fold_identity(mode);
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n_vec; v += stride) {
        const int64_t w0 = v * 4;
        uint4 acc = make_uint4(id, id, id, id);
        for (int32_t t = 0; t < n; ++t) {
            const uint4 x = *reinterpret_cast<const uint4 *>(bitmaps + term_base[t] + w0);
            acc.x = scope_terms::fold_word(acc.x, x.x, mode); acc.y = scope_terms::fold_word(acc.y, x.y, mode);
            acc.z = scope_terms::fold_word(acc.z, x.z, mode); acc.w = scope_terms::fold_word(acc.w, x.w, mode);
        }
        *reinterpret_cast<uint4 *>(dst + w0) = make_uint4(acc.x & scope_terms::tail_mask(w0, n_rows), acc.y & scope_terms::tail_mask(w0 + 1, n_rows),
                                                          acc.z & scope_terms::tail_mask(w0 + 2, n_rows), acc.w & scope_terms::tail_mask(w0 + 3, n_rows));
    }
}

hipError_t launch_scope_terms_combine(const uint32_t *bitmaps, const int64_t *term_base, int32_t n, int32_t mode, int64_t words, int64_t n_rows,
                                      uint32_t *dst, hipStream_t s)
{
    if (n < 1 || !scope_terms::terms_valid(n) || !scope_terms::mode_valid(mode) || words <= 0 || words % 4 != 0 || n_rows < 0 || n_rows > words * 32 ||
        !bitmaps || !term_base || !dst)
        return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(bitmaps) | reinterpret_cast<uintptr_t>(dst)) & 15u) return hipErrorInvalidValue;   // 16-byte vectors
    const int64_t blocks = std::min<int64_t>((words / 4 + 255) / 256, 2048);
    hipLaunchKernelGGL(scope_terms_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bitmaps, term_base, n, mode, words, n_rows, dst);
    return hipGetLastError();
}

// ---- cosine scopes (orr_scope_create_near; the rules are orr_scope_near_plan.h's) -------------------------------------------
static_assert(scope_near::kMaxProbes == kMaxExactQ, "a cosine scope's probes are one walk of the exact dot");

struct NearOut {                       // what the ending of a cosine scope's walk needs
    const double *norm_a;              // [nq] the probes' exact norms
    const double *norm_b;              // [n_rows] the rows' exact norms
    double t;                          // min_cosine
    int32_t mode;
    scope_near::BandEntry *band;       // [band_cap]
    unsigned long long *band_cnt;      // the pairs the walk wanted to list
    int64_t band_cap;
    uint32_t *bm;                      // the scope's bitmap
    int64_t n_rows;
};

// The ending of the walk for the wave's 64 rows [row0, row0 + 64), every lane of the wave taking part: lane l has the exact dots
// acc[0 .. nq) of row row0 + l (zeros at or above n_rows, where the norm counts as 0 as well: cosine 0).  Per pair
// scope_near::cosine_of, per row scope_near::row_state; a pending row (a pair in the band that can still change the fold) lists
// its band pairs for the host and keeps its bit SET until the host has decided (the host clears the losers).  One ballot forms
// the two words, the tail mask clears what is no row, and lane 0 stores the pair: vector stores only.
__device__ __forceinline__ void scope_near_store(const double *acc, int32_t nq, int64_t row0, int lane, const NearOut &o)
{
    const int64_t row = row0 + lane;
    const bool is_row = row < o.n_rows;
    const double nb = is_row ? o.norm_b[row] : 0.0;
    double c[scope_near::kMaxProbes];
#pragma unroll
    for (int q = 0; q < scope_near::kMaxProbes; ++q) {
        c[q] = 0.0;
        if (q < nq) c[q] = scope_near::cosine_of(acc[q], o.norm_a[q], nb);
    }
    const int32_t state = scope_near::row_state(c, nq, o.t, o.mode);
    if (state == scope_near::Pending && is_row) {
#pragma unroll
        for (int q = 0; q < scope_near::kMaxProbes; ++q) {
            if (q < nq && scope_near::in_band(c[q], o.t)) {
                const unsigned long long at = atomicAdd(o.band_cnt, 1ull);
                if (at < (unsigned long long)o.band_cap) {
                    const double d = acc[q];
                    *reinterpret_cast<uint4 *>(o.band + at) = make_uint4((uint32_t)row, (uint32_t)q, (uint32_t)__double2loint(d), (uint32_t)__double2hiint(d));
                }
            }
        }
    }
    const unsigned long long bits = __ballot(state != scope_near::Out);
    if (lane == 0) {
        const int64_t w = row0 >> 5;
        *reinterpret_cast<uint2 *>(o.bm + w) = make_uint2((uint32_t)bits & scope_near::tail_mask(w, o.n_rows),
                                                          (uint32_t)(bits >> 32) & scope_near::tail_mask(w + 1, o.n_rows));
    }
}

// dot_exact_tiled's walk with scope_near_store for its ending: a bit per row where that kernel writes 8 * NQ bytes.  The groups
// run to the end of the BITMAP (words / 2 of them: words % 4 == 0), so every word is written; the walk loads nothing for rows
// at or above n_rows.
template <int NQ>
__global__ __launch_bounds__(256) void scope_near_tiled(const float *__restrict__ E, int32_t D, const float *__restrict__ Q, int64_t words, NearOut o)
{
    exact_walk_tiled<NQ, false, true, true>(E, o.n_rows, words >> 1, D, Q, [&](int64_t row0, int lane, const double (&acc)[NQ]) {
        scope_near_store(acc, NQ, row0, lane, o);
    });
}

// Any D, after dot_exact_generic: one thread per row, plain loads, 64 consecutive rows per wave; the same ending.
__global__ __launch_bounds__(256) void scope_near_generic(const float *__restrict__ E, int32_t D, const float *__restrict__ Q, int32_t nq, int64_t words, NearOut o)
{
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row0 = row & ~(int64_t)63;
    if (row0 >= words * 32) return;                    // (wave-uniform: words * 32 is a multiple of 64)
    double acc[scope_near::kMaxProbes];
#pragma unroll
    for (int q = 0; q < scope_near::kMaxProbes; ++q) {
        acc[q] = 0.0;
        if (q < nq && row < o.n_rows) {
            const float *e = E + row * (int64_t)D, *x = Q + (int64_t)q * D;
            double a = 0.0;
            for (int i = 0; i < D; ++i) {
                float p = x[i] * e[i];
                a += (double)p;
            }
            acc[q] = a;
        }
    }
    scope_near_store(acc, nq, row0, threadIdx.x & 63, o);
}

hipError_t launch_scope_near(const float *E, int64_t n_rows, int32_t D, const float *Q, int32_t nq, const double *norm_a, const double *norm_b,
                             double min_cosine, int32_t mode, scope_near::BandEntry *band, unsigned long long *band_cnt, int64_t band_cap,
                             uint32_t *bm, int64_t words, hipStream_t s)
{
    if (nq < 1 || nq > scope_near::kMaxProbes || D <= 0 || n_rows < 0 || words <= 0 || words % 4 != 0 || n_rows > words * 32 ||
        !scope_near::mode_valid(mode) || min_cosine != min_cosine || !scope_near::band_cap_valid(band_cap) ||
        !E || !Q || !norm_a || !norm_b || !band || !band_cnt || !bm)
        return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(band) & 15u) || (reinterpret_cast<uintptr_t>(bm) & 7u)) return hipErrorInvalidValue;   // 16- and 8-byte stores
    const NearOut o{norm_a, norm_b, min_cosine, mode, band, band_cnt, band_cap, bm, n_rows};
    const bool tiled = (D % 64 == 0) && ((reinterpret_cast<uintptr_t>(E) & 15) == 0);
    if (!tiled) {
        hipLaunchKernelGGL(scope_near_generic, dim3((unsigned)((words * 32 + 255) / 256)), dim3(256), 0, s, E, D, Q, nq, words, o);
        return hipGetLastError();
    }
    const int64_t n_groups = words / 2;
    int64_t blocks = (n_groups + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;          // launch_dot_exact's grid
    dim3 grid((unsigned)blocks), block(256);
#define ORR_LAUNCH_NEAR(NQ_) hipLaunchKernelGGL((scope_near_tiled<NQ_>), grid, block, 0, s, E, D, Q, words, o)
    switch (nq) {
    case 1: ORR_LAUNCH_NEAR(1); break;
    case 2: ORR_LAUNCH_NEAR(2); break;
    case 3: ORR_LAUNCH_NEAR(3); break;
    case 4: ORR_LAUNCH_NEAR(4); break;
    case 5: ORR_LAUNCH_NEAR(5); break;
    case 6: ORR_LAUNCH_NEAR(6); break;
    case 7: ORR_LAUNCH_NEAR(7); break;
    default: ORR_LAUNCH_NEAR(8); break;
    }
#undef ORR_LAUNCH_NEAR
    return hipGetLastError();
}

// out[i] = norm_b[band[i].pos]: the one thing the host's decision of a band pair needs beside the entry and the probe's norm
__global__ __launch_bounds__(256) void scope_near_band_norms_kernel(const scope_near::BandEntry *__restrict__ band, int64_t n,
                                                                    const double *__restrict__ norm_b, int64_t n_rows, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = band[i].pos;
    out[i] = (int64_t)p < n_rows ? norm_b[p] : 0.0;
}

hipError_t launch_scope_near_band_norms(const scope_near::BandEntry *band, int64_t n, const double *norm_b, int64_t n_rows, double *out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    if (!band || !norm_b || !out || n_rows < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scope_near_band_norms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, band, n, norm_b, n_rows, out);
    return hipGetLastError();
}

// ---- cosine range search (orr_search_range_cosine; the rules are orr_range_plan.h's) ----------------------------------------
static_assert(range::kScreenQ == kMaxI8ScreenQ, "a launch group of the range screen is one launch of K2i");

// One kept pair into its query's list: the slot from the list's counter (which counts every kept pair, stored or not), the
// entry as two 16-byte vector stores.
__device__ __forceinline__ void range_list_append(range::ListEntry *__restrict__ list, uint32_t *__restrict__ list_cnt, uint32_t list_cap,
                                                  int64_t row_id, double dot, double nb, uint32_t pos)
{
    const uint32_t slot = atomicAdd(list_cnt, 1u);
    if (slot >= list_cap) return;
    uint4 *o = reinterpret_cast<uint4 *>(list + slot);
    o[0] = make_uint4((uint32_t)row_id, (uint32_t)((unsigned long long)row_id >> 32), (uint32_t)__double2loint(dot), (uint32_t)__double2hiint(dot));
    o[1] = make_uint4((uint32_t)__double2loint(nb), (uint32_t)__double2hiint(nb), pos, 0u);
}

// blockIdx.y = the query; the survivors of its buffer, grid-stride
__global__ __launch_bounds__(256) void range_collect(const SelEntry *__restrict__ buf, const double *__restrict__ buf_dot, const uint32_t *__restrict__ cnt,
                                                     uint32_t cap, const double *__restrict__ norm_a, const double *__restrict__ norm_b,
                                                     const int64_t *__restrict__ row_ids, int64_t n_rows, const double *__restrict__ min_cosine,
                                                     range::ListEntry *__restrict__ list, uint32_t *__restrict__ list_cnt, uint32_t list_cap)
{
    const int b = blockIdx.y;
    const uint32_t n = cnt[b] < cap ? cnt[b] : cap;
    const double na = norm_a[b], t = min_cosine[b];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t pos = buf[(int64_t)b * cap + i].pos;
        if ((int64_t)pos >= n_rows) continue;
        const double dot = buf_dot[(int64_t)b * cap + i], nb = norm_b[pos];
        if (range::device_keeps(scope_near::cosine_of(dot, na, nb), t))
            range_list_append(list + (int64_t)b * list_cap, list_cnt + b, list_cap, row_ids[pos], dot, nb, pos);
    }
}

hipError_t launch_range_collect(const SelEntry *buf, const double *buf_dot, const uint32_t *cnt, uint32_t cap, int32_t nq, const double *norm_a,
                                const double *norm_b, const int64_t *row_ids, int64_t n_rows, const double *min_cosine,
                                range::ListEntry *list, uint32_t *list_cnt, uint32_t list_cap, hipStream_t s)
{
    if (nq <= 0) return hipSuccess;
    if (!buf || !buf_dot || !cnt || cap == 0 || !norm_a || !norm_b || !row_ids || n_rows < 0 || !min_cosine || !list || !list_cnt || list_cap == 0)
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(list) & 15u) return hipErrorInvalidValue;                  // 16-byte stores
    const unsigned blocks = (unsigned)std::min<uint32_t>((cap + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(range_collect, dim3(blocks, (unsigned)nq), dim3(256), 0, s, buf, buf_dot, cnt, cap, norm_a, norm_b, row_ids, n_rows, min_cosine,
                       list, list_cnt, list_cap);
    return hipGetLastError();
}

// One lane per row, grid-stride: the row's word of the allowed bitmap, its norm and id once, then the nq dense dots (consecutive
// lanes, consecutive rows of dots[q]: contiguous loads).
__global__ __launch_bounds__(256) void range_collect_dense(const double *__restrict__ dots, int64_t dot_stride, int32_t nq, const double *__restrict__ norm_a,
                                                           const double *__restrict__ norm_b, const int64_t *__restrict__ row_ids, int64_t n_rows,
                                                           const uint32_t *__restrict__ allowed, const double *__restrict__ min_cosine,
                                                           range::ListEntry *__restrict__ list, uint32_t *__restrict__ list_cnt, uint32_t list_cap)
{
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * 256) {
        if (!((allowed[row >> 5] >> (uint32_t)(row & 31)) & 1u)) continue;
        const double nb = norm_b[row];
        for (int32_t q = 0; q < nq; ++q) {
            const double dot = dots[(int64_t)q * dot_stride + row];
            if (range::device_keeps(scope_near::cosine_of(dot, norm_a[q], nb), min_cosine[q]))
                range_list_append(list + (int64_t)q * list_cap, list_cnt + q, list_cap, row_ids[row], dot, nb, (uint32_t)row);
        }
    }
}

hipError_t launch_range_collect_dense(const double *dots, int64_t dot_stride, int32_t nq, const double *norm_a, const double *norm_b,
                                      const int64_t *row_ids, int64_t n_rows, const uint32_t *allowed, const double *min_cosine,
                                      range::ListEntry *list, uint32_t *list_cnt, uint32_t list_cap, hipStream_t s)
{
    if (nq <= 0 || n_rows <= 0) return hipSuccess;
    if (nq > kMaxExactQ || !dots || dot_stride < n_rows || !norm_a || !norm_b || !row_ids || !allowed || !min_cosine || !list || !list_cnt || list_cap == 0)
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(list) & 15u) return hipErrorInvalidValue;                  // 16-byte stores
    const int64_t blocks = std::min<int64_t>((n_rows + 255) / 256, 2048);
    hipLaunchKernelGGL(range_collect_dense, dim3((unsigned)blocks), dim3(256), 0, s, dots, dot_stride, nq, norm_a, norm_b, row_ids, n_rows, allowed,
                       min_cosine, list, list_cnt, list_cap);
    return hipGetLastError();
}

}  // namespace orr
