// orr_api.hip -- the C ABI of libomnirecall_hip.so (include/omnirecall_hip.h):
// corpus shard management, search orchestration on the index's HIP stream, and
// the host-side exact finish of the k' survivors.
//
// Replaces RecallSearchService.cs:26-37 (GetRecentChunksAsync + Select(ScoreChunk)
// + OrderByDescending/ThenByDescending/Take) for a batch of queries.  There is NO
// CPU scoring path here: without a gfx950 device every compute entry point
// returns ORR_EDEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <chrono>
#include <pthread.h>
#include <dlfcn.h>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <cstring>
#include <limits>
#include <mutex>
#include <shared_mutex>
#include <deque>
#include <new>
#include <numeric>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "orr_escalation.h"
#include "orr_insert_plan.h"
#include "orr_kernels.h"
#include "orr_keyword_plan.h"
#include "orr_lanes.h"
#include "orr_scope_plan.h"
#include "orr_mask_plan.h"
#include "orr_group_plan.h"
#include "orr_scope_set_plan.h"
#include "orr_scope_terms_plan.h"
#include "orr_scope_near_plan.h"
#include "orr_range_bulk_plan.h"
#include "orr_cluster_handle_plan.h"
#include "orr_cluster_group_plan.h"
#include "orr_cluster_scope_plan.h"
#include "orr_cluster_diverse_plan.h"
#include "orr_cluster_per_key_plan.h"
#include "orr_routed_plan.h"
#include "orr_token_index.h"

namespace {

thread_local std::string g_last_error = "";

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(_e == hipErrorOutOfMemory ? ORR_ENOMEM : ORR_EDEVICE, "%s failed: %s (%s:%d)", \
                        #expr, hipGetErrorString(_e), __FILE__, __LINE__);                            \
    } while (0)

#define ORR_TRY(expr)          \
    do {                       \
        int _r = (expr);       \
        if (_r != ORR_OK) return _r; \
    } while (0)

// Grow-only device buffer.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return ORR_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(ORR_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return ORR_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// Grow-only pinned host buffer (device-visible): small uploads, the query copy, and the
// candidate records the last kernel writes straight into host memory.
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return ORR_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(ORR_ENOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return ORR_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct KernelStat {
    std::string name;
    int64_t launches = 0;
    double total_ms = 0.0;
    double algo_bytes = 0.0;
};

struct PendingEvent {
    int stat;
    hipEvent_t start, stop;
};

// orr_index_capture_screen: what the first two-stage pass after the arming left in front of its exact tail, on the handle.
struct ScreenCapture {
    std::atomic<int> armed{0};
    bool have = false;
    orr_screen_capture info{};
    std::vector<unsigned long long> floor_key;
    std::vector<double> L;
    std::vector<uint32_t> cnt;
    std::vector<orr::SelEntry> buf;
};

// What the last keyword chain on a lane left clean, so that the next one clears only what nobody has vouched for.  The chain
// withdraws everything on entry (launch_keyword_side) and its caller grants it again behind the clean (clean_keyword_side);
// each voucher names the buffer it is about, which may have moved since.  A chain whose caller never cleaned finds nothing
// granted and clears everything itself: slow, not wrong.
struct KwVouchers {
    size_t bitmaps = 0;                // leading bytes of ws_bitmaps known to be zero
    const void *bitmaps_of = nullptr;
    bool counters = false;             // the hit counter and the per-term hit counts are zero
    const void *counters_of[2] = {nullptr, nullptr};   // ws_counter, ws_kwalias
    bool clear_in_flight = false;      // the bitmaps' clearing is on the auxiliary stream: ev_bm_clean is recorded behind it.  No
                                       // voucher but a debt -- the next chain to write the bitmaps waits for it -- so it outlives withdraw
    KwVouchers withdraw()
    {
        const KwVouchers held = *this;
        *this = KwVouchers{};
        clear_in_flight = held.clear_in_flight;
        return held;
    }
    void withdraw_bitmaps() { bitmaps = 0; bitmaps_of = nullptr; }      // compaction, insertion: the rows moved
    void grant_bitmaps(const void *buf, size_t bytes, bool on_aux_stream)
    {
        bitmaps = bytes;
        bitmaps_of = buf;
        if (on_aux_stream) clear_in_flight = true;
    }
    void grant_counters(const void *counter, const void *alias_counts)
    {
        counters = true;
        counters_of[0] = counter;
        counters_of[1] = alias_counts;
    }
};

}  // namespace

struct orr_index {
    int device = 0;
    int32_t dim = 0;
    int64_t row_base = 0;
    hipStream_t stream = nullptr;      // main stream: dots, fused score, selection
    hipStream_t stream_kw = nullptr;   // keyword scan runs beside the HBM-bound dot kernel
    hipStream_t stream_aux = nullptr;  // what must not sit in front of the keyword chain: the clearing of the term bitmaps behind a
                                       // search (0.1 ms at 10M rows x 256 queries) and the norms of device-resident queries
    hipEvent_t ev_bm_clean = nullptr;  // ... recorded behind that clearing; the next search's posting expansion waits for it
    KwVouchers kw_clean;               // what the last keyword chain on this lane left clean
    hipEvent_t ev_inputs = nullptr, ev_kw_done = nullptr, ev_main_ready = nullptr, ev_range[15] = {};     // (one per row range but the first: 16 ranges at most)
    std::mutex mu;

    // corpus, in append order until seal, in candidate order afterwards
    int64_t n_rows = 0, cap_rows = 0;
    float *d_emb = nullptr;
    int64_t *d_created = nullptr;
    int64_t *d_row_ids = nullptr;
    // lowercased content: row r = d_pool[d_cstart[r] .. +d_clen[r]), starts 16-byte aligned,
    // each row followed by 1..16 spaces (see keyword_scan_kernel)
    uint64_t *d_cstart = nullptr;      // [cap_rows]
    uint32_t *d_clen = nullptr;        // [cap_rows]
    uint8_t *d_pool = nullptr;
    uint64_t pool_len = 0, pool_cap = 0;
    double *d_norm_b = nullptr;
    // after seal the raw content is replaced by the token index (orr_token_index.cpp)
    int64_t n_tokens = 0;
    uint8_t *d_vpool = nullptr;        // vocabulary in the scan kernel's row layout
    uint64_t *d_vstart = nullptr;      // [n_tokens]
    uint32_t *d_vlen = nullptr;        // [n_tokens]
    uint64_t *d_post_off = nullptr;    // [n_tokens+1]
    uint32_t *d_post_rows = nullptr;   // ascending candidate positions per token
    uint64_t n_postings = 0;
    // vocabulary tokens longer than 16 bytes (URLs and the like) go through the wave-per-token scan; the rest is
    // matched one lane per token.  Built at the first search with terms (ensure_vlong); -1 = not yet.
    int64_t n_vlong = -1;
    int64_t n_vmid = 0;                // the first n_vmid entries of the list are the tokens of 17..32 bytes (one lane per token too)
    DevBuf vlong_start, vlong_len, vlong_id;
    // stored row bitmaps of the FREQUENT vocabulary tokens (a posting list of at least rows / 64 entries: the bitmap is at most
    // twice its bytes), built at the first search with terms over a large shard (ensure_token_bitmaps): a query term whose only
    // hit is such a token uses the stored bitmap as it is instead of expanding the posting list again for every batch
    int64_t n_tok_bm = -1;             // -1: not looked at yet; 0: none
    int64_t tok_bm_words = 0;
    DevBuf tok_bm, tok_bm_index;       // [n_tok_bm][tok_bm_words] u32; [n_tokens] int32 bitmap number or -1
    std::vector<int64_t> h_created;    // host mirror (seal-time ordering)
    std::vector<uint32_t> h_clen;      // host mirror of content lengths
    std::vector<uint64_t> h_cprefix;   // after seal: bytes of content in rows [0, r)
    std::vector<double> h_norm_a;      // exact query norms of the batch in flight (run_shard -> host finish)
    std::vector<uint32_t> h_survivors; // two-stage pass: (query,row) pairs the screen kept, per query of the batch in flight (else empty)
    uint32_t kw_hits_cap = 16u << 20;  // (term, token) matches the hit list of the keyword chain holds; grows to the measured count when a batch exceeds it
    // orr_index_keyword_bitmaps, for the one chain it runs on this lane: the short-token form (-1 as a search chooses, 0 all-pairs,
    // 1 lookup) and the 17..32-byte kernel (-1 default, 0 off) ahead of the environment switches; and the form the last chain ran
    int kw_force_form = -1, kw_force_mid = -1, kw_form_ran = -1;
    uint32_t survivor_cap = 8192;      // entries per query of the survivors' buffers; grows when a query overflows it (clustered corpora)
    uint32_t pass_cap = 8192;          // what the pass in flight uses: survivor_cap, halved until a batch's buffers stay below 2 GiB
    orr_search_stats sstats{};         // orr_index_search_stats
    bool sealed = false;
    bool is_view = false;              // a second search lane over another index's sealed corpus (orr_index_view)
    bool opt_fuse_epilogue = false;
    int opt_two_stage = 1;             // 0 off, 1 on (bf16 shadow when it fits), 2 on without the shadow
    int opt_shard_pass = 0;            // orr_search_shard: 0 the library picks the pass, 1 unfused batched pass, 2 exact pass
    int opt_shard_topk = 0;            // orr_search_shard: the caller's topK when > 0 (the two-stage floor then comes from the k-th best, not the k'-th)
    int sample_boost = 1;              // two-stage pass: the sampled prefix is this many times the default (1..16), steered by the survivors measured
    DevBuf emb_shadow;                 // bf16(E), [n_rows][dim]: operand of the screening GEMM (two-stage pass)
    bool shadow_ready = false, shadow_failed = false;
    DevBuf emb_i8, i8_scale, i8_rel_err, i8_rel_hat, i8_rowf;   // int8 shadow: streaming screen of 1..4 queries (K2i), screening GEMM (K2j)
    bool i8_ready = false, i8_failed = false;
    // deleted rows (orr_index_delete_rows): ascending positions, mirrored on the device for the record flags
    std::vector<int64_t> dead;
    DevBuf d_dead;
    int64_t dead_before = 0;           // deleted rows in the shards in front of this one ("dead_rows_before")
    const orr_index *parent = nullptr; // views: the deleted set lives in the owning index
    std::vector<std::pair<int64_t, int64_t>> id_index;   // (row id, position) ascending, built at the first delete

    // scoped search (orr_search_batch_scoped): the shard's (row id, position) pairs sorted by id, on the OWNING index -- built at
    // the first scoped search (ensure_scope_table), shared by its lanes and views, dropped when positions move (compact, insert)
    std::mutex scope_mu;
    std::atomic<bool> scope_ready{false};
    int64_t *scope_tab_ids = nullptr;  // [n_rows] ascending
    uint32_t *scope_tab_pos = nullptr; // [n_rows] positions, ascending within equal ids
    DevBuf ws_scope_ids, ws_scope_meta, ws_scope_bm, ws_scope_chunks, ws_scope_sel;   // a lane's: listed ids, offsets + limits, bitmaps, chunk counts, a pass's queries
    PinnedBuf pin_scope, pin_scope_pass;
    DevBuf ws_scope_terms;                     // a lane's: where each distinct term's bitmap starts (orr_scope_create_terms)
    PinnedBuf pin_scope_terms;                 // ... and the host's copy of it
    // cosine scopes (orr_scope_create_near), a lane's: the probes and their exact norms, the band list with its counter, the
    // listed rows' norms (then the positions the host decided out)
    DevBuf ws_near_q, ws_near_norm, ws_near_band, ws_near_cnt, ws_near_rows;
    int64_t near_band_cap = scope_near::kDefaultBandCap;   // "near_band_cap": entries of the band list; grows to the measured count when a walk exceeds it
    // cosine range search (orr_search_range_cosine), a lane's: the allowed rows of a call without a scope; the queries as given
    // and in their walked order; their exact norms; per walked query norm, threshold and QueryConst; the survivors' and the
    // lists' counters; the survivors' buffers with their exact dots; the lists; the exact form's dense dots
    DevBuf ws_range_allowed, ws_range_q, ws_range_qp, ws_range_norm, ws_range_consts, ws_range_cnt, ws_range_buf, ws_range_bdot, ws_range_list, ws_range_dots, ws_range_args;
    // diverse search (orr_search_batch_diverse, orr_index_pair_dots), a lane's: the lists' positions and lengths, the pair matrices;
    // pinned: the staging of the first two and the matrices as they come back
    DevBuf ws_diverse_pos, ws_diverse_cnt, ws_diverse_out;
    PinnedBuf pin_diverse;
    // ... over a cluster (orr_cluster_search_batch_diverse, orr_cluster_pair_dots), a lane's: as a source the positions it gathers
    // and the gathered rows, pinned: the rows on their way to the other shards; as a home the rows the others sent, the lists' masks
    DevBuf ws_diverse_gpos, ws_diverse_gather, ws_diverse_foreign, ws_diverse_mask;
    PinnedBuf pin_diverse_rows;
    int opt_range_gemm = range_bulk::Auto;                 // "range_gemm" (orr_search_range_cosine_bulk): 0 the GEMM screen from 65 walked queries up, 1 wherever it applies, 2 never
    int opt_range_form = range::Auto;                      // "range_form": 0 the screen where it applies, 1 the same, 2 the exact form only
    int64_t opt_range_pair_cap = range::kDefaultPairCap;   // "range_pair_cap": kept pairs of one query beyond which the call is ORR_ELIMIT
    int64_t range_buffer = range::kDefaultBuffer;          // "range_buffer": entries per query of the survivors' buffers and the lists; grows to the measured count
    int64_t range_list_cap = 0;                            // ... and what the exact form's lists have grown to beyond it
    // masked search (orr_search_batch_masked), a lane's: the call's shared scope bitmap and its chunk counts (the list path in
    // parts rewrites ws_scope_bm per part), the sample's counts and the zeros that select the one bitmap, n_clip and the sample's sizes
    DevBuf ws_mask_bm, ws_mask_chunks, ws_mask_cnt, ws_mask_meta;
    PinnedBuf pin_mask;
    // grouped masked search (orr_search_batch_masked_groups), a lane's: the call's G bitmaps and their chunk counts (a group's
    // own masked call rewrites ws_scope_bm and ws_mask_bm), the groups' clips and samples; pinned: the clips as mask_clip leaves them
    DevBuf ws_group_bm, ws_group_chunks, ws_group_meta;
    PinnedBuf pin_group;
    // scope handles (orr_scope) of this shard, on the OWNING index, under scope_mu: deletes clear their rows, compaction and
    // insertion carry them along, orr_index_destroy orphans them
    std::vector<orr_scope *> scopes;
    // row keys (orr_keys) of this shard, registered like the scopes, under scope_mu: compaction and insertion carry them along
    // (KeysRemap), orr_index_destroy orphans them
    std::vector<orr_keys *> key_cols;
    int opt_mask_screen = 0;          // "mask_screen": 0 by the cost rule, 1 whenever eligible, 2 never (orr_mask_plan.h)
    int64_t opt_mask_part_rows = mask::kDefaultPartRows;   // "mask_part_rows": scoped rows per part of the list path
    int64_t opt_key_groups_slice = 0;                      // "key_groups_slice": keys per slice of orr_keys_centroids' sums; 0 by key_groups::slice_keys

    // search workspace
    DevBuf ws_q, ws_dot, ws_dotf, ws_sel, ws_cand, ws_qc, ws_rowc, ws_tau, ws_qsplit, ws_fcnt, ws_fbuf, ws_fqf, ws_fany, ws_tsL, ws_tskey, ws_qtiled, ws_fdot, ws_pbuf, ws_psel, ws_q8, ws_q8s1, ws_q8err, ws_zero, ws_norm_a;
    DevBuf ws_keys_a, ws_keys_b, ws_vals_a, ws_vals_b, ws_sort_tmp, ws_raw, ws_src_start, ws_qsub;
    DevBuf ws_vmatch, ws_bitmaps, ws_hits, ws_counter, ws_meta, ws_tickets, ws_kwalias;
    PinnedBuf pin_meta, pin_q, pin_qc, pin_cand, pin_norm, pin_cnt, pin_kwcnt;
    hipEvent_t ev_q = nullptr;

    // search lanes (owning index only; orr_lanes.h): concurrent searches on ONE handle each take a lane of this pool
    LanePool lanes{this};
    bool internal_lane = false;            // this view belongs to its parent's lane pool (not handed to the caller)
    std::atomic<int> user_views{0};        // views handed to the caller (orr_index_view) that are still alive: they pin the shard's layout

    // orr_index_capture_screen, on the handle the caller holds (a lane of the pool records into its owner's)
    ScreenCapture capture;

    // profiling
    int profiling = 0;                     // 0 off, 1 every kernel, 2 only the pass over all rows (the kernel a roofline is quoted on)
    std::vector<KernelStat> stats;
    std::vector<PendingEvent> pending;
    std::vector<hipEvent_t> event_pool;
};

// A scope handle: a set of rows of one sealed shard as the bitmap scope_lookup writes (words % 4 == 0, deleted rows left out,
// bits at or above n_rows clear), with what a masked search asks of a resolved scope.  Every operation keeps all of it current
// (refresh_scope).  Searches hold mu shared; whatever writes the bitmap holds it exclusively.
struct orr_scope {
    std::atomic<orr_index *> owner{nullptr};   // the owning index; nullptr once that was destroyed (the handle is orphaned)
    mutable std::shared_mutex mu;
    int64_t n_rows = 0, words = 0;             // the shard's rows the bitmap covers, its words (scope::bitmap_bytes / 4)
    uint32_t *bm = nullptr;                    // device [words]
    uint32_t *chunks = nullptr;                // device [scope_chunks(words)], as launch_scope_counts leaves them
    std::atomic<int64_t> live{0};              // set bits
    int64_t n_clip_all = 0;                    // one past the last set bit
};

// Row keys: one int64 per row of one sealed shard (ORR_KEY_NONE: no key), resident on its device.  Lifetime and threads are a
// scope's: searches hold mu shared, orr_keys_set and orr_keys_destroy hold it exclusively, maintenance swaps the column under it.
struct orr_keys {
    std::atomic<orr_index *> owner{nullptr};   // the owning index; nullptr once that was destroyed (the handle is orphaned)
    mutable std::shared_mutex mu;
    int64_t n_rows = 0;                        // the shard's rows the column covers
    int64_t *d_key = nullptr;                  // device [max(n_rows, 1)]
};

// orr_scope_destroy and the orphaning in orr_index_destroy exclude each other, whatever threads release the two handles: a
// scope's destroy either finishes before its index lets go of it or finds itself orphaned.  Taken before scope_mu and a scope's mu.
static std::mutex g_scope_life_mu;

static int make_view(orr_index *parent, orr_index **out, bool internal);

namespace {

// ---- search lanes (orr_lanes.h) --------------------------------------------------------------------------------------
// The request path is concurrent by nature (RecallSearchService is scoped, one instance per request, Program.cs:59; the store
// behind it is lock-free, InMemoryIngestionStore.cs:8-9).  A search on an OWNING index takes a free lane: the index's own
// workspaces, or those of an internal view (created on demand, at most max_lanes - 1 of them; corpus and shadows are shared,
// nothing is copied).  Searches from different threads on one handle then run side by side; the caller never sees a view.
// A view handle the caller made itself (orr_index_view) is its own single lane, as before.
LanePool *pool_of(orr_index *idx) { return idx && !idx->is_view ? &idx->lanes : nullptr; }

// how the pool of `idx` makes another lane; none before the seal
LanePool::Make lane_maker(orr_index *idx)
{
    if (!idx->sealed) return {};
    return [idx](orr_index **v) { return make_view(idx, v, true); };   // (waits for the search that holds the index's own lane)
}

// a lane starts from the survivors' buffer size that another lane of its handle measured
void adopt_survivor_hint(orr_index *owner, orr_index *lane)
{
    const uint32_t hint = owner->lanes.shared().survivor_cap_hint;
    if (hint > lane->survivor_cap) lane->survivor_cap = hint;
}

void publish_survivor_hint(orr_index *owner, uint32_t cap)
{
    owner->lanes.update_shared([cap](LanePool::Shared &sh) { sh.survivor_cap_hint = std::max(sh.survivor_cap_hint, cap); });
}

Lane acquire_lane(orr_index *idx)
{
    if (idx->is_view) return Lane::of(idx);
    Lane ln = idx->lanes.acquire(lane_maker(idx));
    adopt_survivor_hint(idx, ln.lane);
    return ln;
}

// fn(lane) for the index and every internal view of it; the caller holds Exclusive
template <class F> void for_each_lane(orr_index *idx, F &&fn)
{
    if (idx->is_view) fn(idx);
    else idx->lanes.for_each_lane(fn);
}

int stat_slot(orr_index *idx, const char *name)
{
    for (size_t i = 0; i < idx->stats.size(); ++i)
        if (idx->stats[i].name == name) return (int)i;
    KernelStat s;
    s.name = name;
    idx->stats.push_back(s);
    return (int)idx->stats.size() - 1;
}

hipEvent_t take_event(orr_index *idx)
{
    if (!idx->event_pool.empty()) {
        hipEvent_t e = idx->event_pool.back();
        idx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// Brackets one launch with events on the index's stream when profiling is on.
struct Timed {
    // the one launch per search that streams every row (an event pair costs a few microseconds of stream time each, which a
    // one-query search notices: level 2 times just this kernel)
    static bool over_all_rows(const char *name)
    {
        return (strncmp(name, "screen_", 7) == 0 && !strstr(name, "prefix")) || strncmp(name, "gemm_dot", 8) == 0 ||
               strcmp(name, "dot_exact") == 0 || strcmp(name, "gemv_mfma") == 0;
    }
    orr_index *idx;
    PendingEvent pe;
    bool on;
    hipStream_t st;
    Timed(orr_index *i, const char *name, double algo_bytes, hipStream_t stream = nullptr)
        : idx(i), on(i->profiling == 1 || (i->profiling == 2 && over_all_rows(name))), st(stream ? stream : i->stream)
    {
        if (!on) return;
        pe.stat = stat_slot(idx, name);
        idx->stats[pe.stat].algo_bytes += algo_bytes;
        pe.start = take_event(idx);
        pe.stop = take_event(idx);
        (void)hipEventRecord(pe.start, st);
    }
    ~Timed()
    {
        if (!on) return;
        (void)hipEventRecord(pe.stop, st);
        idx->pending.push_back(pe);
    }
};

// After a stream synchronise: fold the finished event pairs into the counters.
void collect_events(orr_index *idx)
{
    for (auto &pe : idx->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pe.start, pe.stop) == hipSuccess) {
            idx->stats[pe.stat].launches += 1;
            idx->stats[pe.stat].total_ms += (double)ms;
        }
        idx->event_pool.push_back(pe.start);
        idx->event_pool.push_back(pe.stop);
    }
    idx->pending.clear();
}

int bind_device(const orr_index *idx)
{
    HIP_TRY(hipSetDevice(idx->device));
    return ORR_OK;
}

template <typename T> int dev_alloc(T **out, size_t count)
{
    *out = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(out), count * sizeof(T));
    if (e != hipSuccess) {
        *out = nullptr;
        return fail(ORR_ENOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    }
    return ORR_OK;
}

// Reallocates a device array keeping the first `keep` elements.
template <typename T> int dev_grow(T **buf, size_t keep, size_t new_count, hipStream_t s)
{
    T *nb = nullptr;
    ORR_TRY(dev_alloc(&nb, new_count));
    if (*buf && keep) {
        hipError_t e = hipMemcpyAsync(nb, *buf, keep * sizeof(T), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(nb);
            return fail(ORR_EDEVICE, "device copy failed: %s", hipGetErrorString(e));
        }
    }
    if (*buf) (void)hipFree(*buf);
    *buf = nb;
    return ORR_OK;
}

int ensure_row_capacity(orr_index *idx, int64_t rows)
{
    if (rows <= idx->cap_rows) return ORR_OK;
    int64_t nc = std::max<int64_t>(rows, idx->cap_rows + idx->cap_rows / 2);
    nc = std::max<int64_t>(nc, 1024);
    if (idx->dim > 0) ORR_TRY(dev_grow(&idx->d_emb, (size_t)idx->n_rows * idx->dim, (size_t)nc * idx->dim, idx->stream));
    ORR_TRY(dev_grow(&idx->d_created, (size_t)idx->n_rows, (size_t)nc, idx->stream));
    ORR_TRY(dev_grow(&idx->d_row_ids, (size_t)idx->n_rows, (size_t)nc, idx->stream));
    ORR_TRY(dev_grow(&idx->d_cstart, (size_t)idx->n_rows, (size_t)nc, idx->stream));
    ORR_TRY(dev_grow(&idx->d_clen, (size_t)idx->n_rows, (size_t)nc, idx->stream));
    idx->cap_rows = nc;
    return ORR_OK;
}

int ensure_pool_capacity(orr_index *idx, uint64_t bytes)
{
    if (bytes + orr::kScanPoolSlack <= idx->pool_cap) return ORR_OK;
    uint64_t nc = std::max<uint64_t>(bytes + orr::kScanPoolSlack, idx->pool_cap + idx->pool_cap / 2);
    nc = std::max<uint64_t>(nc, 1u << 16);
    ORR_TRY(dev_grow(&idx->d_pool, (size_t)idx->pool_len, (size_t)nc, idx->stream));
    idx->pool_cap = nc;
    return ORR_OK;
}

// Exact sum_i (double)fl32(q_i*q_i) in index order: normA of RecallSearchService.cs:80.
double exact_norm(const float *q, int32_t dim)
{
    double acc = 0.0;
    for (int32_t i = 0; i < dim; ++i) {
        float p = q[i] * q[i];
        acc += (double)p;
    }
    return acc;
}

// A few persistent host threads for the per-query work around a batch (exact norms of host-resident queries, the
// host finish): queries are independent, and starting threads per call costs more than the work of a small batch.
// One parallel region at a time; a second caller (another search lane) simply runs its tasks itself.
class HostPool {
public:
    static HostPool &get()
    {
        static HostPool *pool = new HostPool((int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency())) - 1);
        return *pool;                                  // never destroyed: its threads sleep until the process ends
    }
    int width() const { return (int)workers_.size() + 1; }
    void run(int n_tasks, const std::function<void(int)> &fn)
    {
        std::unique_lock<std::mutex> region(region_mu_, std::try_to_lock);
        if (!region.owns_lock() || workers_.empty() || n_tasks <= 1 || forked_.load(std::memory_order_relaxed)) {
            for (int i = 0; i < n_tasks; ++i) fn(i);
            return;
        }
        {
            std::lock_guard<std::mutex> l(mu_);
            fn_ = &fn; n_tasks_ = n_tasks; next_.store(0); active_ = (int)workers_.size(); ++generation_;
        }
        cv_work_.notify_all();
        for (int i; (i = next_.fetch_add(1)) < n_tasks;) fn(i);
        std::unique_lock<std::mutex> l(mu_);
        cv_done_.wait(l, [&] { return active_ == 0; });
    }

private:
    explicit HostPool(int n_workers)
    {
        for (int i = 0; i < n_workers; ++i) workers_.emplace_back([this] { loop(); });
        for (auto &w : workers_) w.detach();
        // a forked child inherits this object but none of its threads: there every region runs in the caller
        pthread_atfork(nullptr, nullptr, [] { forked_.store(true); });
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> l(mu_);
            cv_work_.wait(l, [&] { return generation_ != seen; });
            seen = generation_;
            const std::function<void(int)> *fn = fn_;
            const int n = n_tasks_;
            l.unlock();
            for (int i; (i = next_.fetch_add(1)) < n;) (*fn)(i);
            l.lock();
            if (--active_ == 0) cv_done_.notify_one();
        }
    }
    static inline std::atomic<bool> forked_{false};
    std::mutex region_mu_, mu_;
    std::condition_variable cv_work_, cv_done_;
    std::vector<std::thread> workers_;
    const std::function<void(int)> *fn_ = nullptr;
    int n_tasks_ = 0, active_ = 0;
    std::atomic<int> next_{0};
    uint64_t generation_ = 0;
};

// The same sums for a batch.  Each query's sum is a chain of dependent fp64 additions (the order is
// part of the reference's arithmetic), so eight queries are walked in lock step to keep the adder busy.
void exact_norms_range(const float *q, int32_t B, int32_t dim, double *out);
void exact_norms(const float *q, int32_t B, int32_t dim, double *out)
{
    if ((int64_t)B * dim < (1 << 18)) { exact_norms_range(q, B, dim, out); return; }
    const int32_t groups = (B + 7) / 8;                 // groups of eight queries, shared out over the pool
    HostPool::get().run(groups, [&](int g) {
        const int32_t b0 = g * 8, nb = std::min<int32_t>(8, B - b0);
        exact_norms_range(q + (size_t)b0 * dim, nb, dim, out + b0);
    });
}

void exact_norms_range(const float *q, int32_t B, int32_t dim, double *out)
{
    int32_t b = 0;
    for (; b + 8 <= B; b += 8) {
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const float *r = q + (size_t)b * dim;
        for (int32_t i = 0; i < dim; ++i)
            for (int j = 0; j < 8; ++j) {
                float p = r[(size_t)j * dim + i] * r[(size_t)j * dim + i];
                acc[j] += (double)p;
            }
        for (int j = 0; j < 8; ++j) out[b + j] = acc[j];
    }
    for (; b < B; ++b) out[b] = exact_norm(q + (size_t)b * dim, dim);
}

// double.CompareTo
int compare_double(double a, double b)
{
    if (a < b) return -1;
    if (a > b) return 1;
    if (a == b) return 0;
    if (std::isnan(a)) return std::isnan(b) ? 0 : -1;
    return 1;
}

struct Ranked {
    double score;
    int64_t order_key;
    int64_t row_id;
};

// RecallSearchService.cs:59-67 for one surviving candidate, in the reference's own
// arithmetic on the host (libm exp = what Math.Exp calls), from the exact pieces
// the device produced.
double exact_score(const orr_candidate &c, bool use_cos, double norm_a, int32_t n_terms, int64_t now_ticks)
{
    double cosv = 0.0;
    if (use_cos)
        cosv = scope_near::cosine_of(c.dot, norm_a, c.norm_b);   // :84-87, the one expression the cosine scope's band decides with too
    double kw = n_terms > 0 ? (double)c.matches / (double)n_terms : 0.0;
    double total_days = (double)(now_ticks - c.created_ticks) / 864000000000.0;
    double age_days = total_days > 0.0 ? total_days : 0.0;
    double rec = std::exp(-age_days / 30.0);
    return (cosv * 0.7) + (kw * 0.2) + (rec * 0.1);
}

// Absolute slack between the device's selection score and the exact host score
// of the same row: identical IEEE operations except exp (ocml vs libm, a few ulp
// of a value <= 1, times 0.1).
constexpr double kCertifyEps = 1e-13;

}  // namespace

namespace {

// Shard file -> device array whose values index something (orr_index_load): every element is checked on its way through the host buffer
// (a shard file is input: posting rows >= n_rows would make expand_hits write outside the term bitmaps).
template <typename T, typename CHECK>
int read_device_array_checked(FILE *f, T *dptr, size_t count, std::vector<uint8_t> &buf, CHECK ok_run, const char *what)
{
    const size_t per = buf.size() / sizeof(T);
    for (size_t off = 0; off < count; off += per) {
        const size_t m = std::min(per, count - off);
        if (fread(buf.data(), sizeof(T), m, f) != m) return fail(ORR_EINVAL, "shard file is truncated");
        if (!ok_run(reinterpret_cast<const T *>(buf.data()), off, m)) return fail(ORR_EINVAL, "shard file: malformed %s", what);
        HIP_TRY(hipMemcpy(dptr + off, buf.data(), m * sizeof(T), hipMemcpyHostToDevice));
    }
    return ORR_OK;
}

}  // namespace

// the events that release the later row ranges' count words (one per range but the first)
static bool create_range_events(hipEvent_t (&ev)[15])
{
    for (hipEvent_t &e : ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
    return true;
}

extern "C" {

int orr_abi_version(void) { return ORR_ABI_VERSION; }

const char *orr_last_error(void) { return g_last_error.c_str(); }

int orr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

int orr_index_create(const orr_config *cfg, orr_index **out)
{
    if (!cfg || !out) return fail(ORR_EINVAL, "orr_index_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(orr_config)) return fail(ORR_EINVAL, "orr_config.struct_size mismatch");
    if (cfg->dim < 0 || cfg->capacity_rows < 0 || cfg->row_base < 0) return fail(ORR_EINVAL, "negative size in orr_config");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(ORR_EDEVICE, "no HIP device available: libomnirecall_hip has no CPU path");
    if (cfg->device < 0 || cfg->device >= n_dev) return fail(ORR_EINVAL, "device %d out of range (%d visible)", cfg->device, n_dev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ORR_EDEVICE, "device %d is %s; this library carries gfx950 code only", cfg->device, prop.gcnArchName);
    orr_index *idx = new (std::nothrow) orr_index();
    if (!idx) return fail(ORR_ENOMEM, "out of host memory");
    idx->device = cfg->device;
    idx->dim = cfg->dim;
    idx->row_base = cfg->row_base;
    if (hipSetDevice(idx->device) != hipSuccess || hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&idx->stream_kw, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&idx->stream_aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&idx->ev_bm_clean, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&idx->ev_inputs, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&idx->ev_kw_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&idx->ev_main_ready, hipEventDisableTiming) != hipSuccess ||
        !create_range_events(idx->ev_range) ||
        hipEventCreateWithFlags(&idx->ev_q, hipEventDisableTiming) != hipSuccess) {
        orr_index_destroy(idx);
        return fail(ORR_EDEVICE, "cannot create streams on device %d", cfg->device);
    }
    if (cfg->capacity_rows > 0) {
        int r = ensure_row_capacity(idx, cfg->capacity_rows);
        if (r != ORR_OK) { orr_index_destroy(idx); return r; }
    }
    *out = idx;
    return ORR_OK;
}

void orr_index_destroy(orr_index *idx)
{
    if (!idx) return;
    if (idx->is_view && !idx->internal_lane && idx->parent) const_cast<orr_index *>(idx->parent)->user_views.fetch_sub(1);
    if (!idx->is_view) {                               // the internal lanes go first (they borrow the corpus)
        std::vector<orr_index *> views;
        {
            LanePool::Exclusive all(&idx->lanes);
            views = idx->lanes.drain();
            idx->lanes.set_max_lanes(1);
        }
        for (orr_index *l : views) orr_index_destroy(l);
    }
    (void)hipSetDevice(idx->device);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    if (idx->stream_kw) (void)hipStreamSynchronize(idx->stream_kw);
    if (idx->stream_aux) (void)hipStreamSynchronize(idx->stream_aux);
    if (idx->ev_bm_clean) (void)hipEventDestroy(idx->ev_bm_clean);
    if (idx->stream_aux) (void)hipStreamDestroy(idx->stream_aux);
    if (idx->ev_inputs) (void)hipEventDestroy(idx->ev_inputs);
    if (idx->ev_kw_done) (void)hipEventDestroy(idx->ev_kw_done);
    if (idx->ev_main_ready) (void)hipEventDestroy(idx->ev_main_ready);
    for (hipEvent_t e : idx->ev_range) if (e) (void)hipEventDestroy(e);
    if (idx->stream_kw) (void)hipStreamDestroy(idx->stream_kw);
    for (auto &pe : idx->pending) { (void)hipEventDestroy(pe.start); (void)hipEventDestroy(pe.stop); }
    for (auto e : idx->event_pool) (void)hipEventDestroy(e);
    if (!idx->is_view) {                               // a view borrows the corpus and the shadow
        if (idx->d_emb) (void)hipFree(idx->d_emb);
        if (idx->d_created) (void)hipFree(idx->d_created);
        if (idx->d_row_ids) (void)hipFree(idx->d_row_ids);
        if (idx->d_cstart) (void)hipFree(idx->d_cstart);
        if (idx->d_clen) (void)hipFree(idx->d_clen);
        if (idx->d_pool) (void)hipFree(idx->d_pool);
        if (idx->d_norm_b) (void)hipFree(idx->d_norm_b);
        if (idx->d_vpool) (void)hipFree(idx->d_vpool);
        if (idx->d_vstart) (void)hipFree(idx->d_vstart);
        if (idx->d_vlen) (void)hipFree(idx->d_vlen);
        if (idx->d_post_off) (void)hipFree(idx->d_post_off);
        if (idx->d_post_rows) (void)hipFree(idx->d_post_rows);
        if (idx->scope_tab_ids) (void)hipFree(idx->scope_tab_ids);
        if (idx->scope_tab_pos) (void)hipFree(idx->scope_tab_pos);
        // scope handles that are still alive lose their device memory and their shard: every later call on one is ORR_ESTATE
        std::lock_guard<std::mutex> life(g_scope_life_mu);
        std::lock_guard<std::mutex> g(idx->scope_mu);
        for (orr_scope *sc : idx->scopes) {
            std::unique_lock<std::shared_mutex> w(sc->mu);
            if (sc->bm) (void)hipFree(sc->bm);
            if (sc->chunks) (void)hipFree(sc->chunks);
            sc->bm = nullptr; sc->chunks = nullptr;
            sc->live.store(-1);
            sc->owner.store(nullptr);
        }
        idx->scopes.clear();
        for (orr_keys *k : idx->key_cols) {            // row keys likewise
            std::unique_lock<std::shared_mutex> w(k->mu);
            if (k->d_key) (void)hipFree(k->d_key);
            k->d_key = nullptr;
            k->owner.store(nullptr);
        }
        idx->key_cols.clear();
    } else {
        idx->emb_shadow.p = nullptr; idx->emb_shadow.cap = 0;
        for (DevBuf *b : {&idx->emb_i8, &idx->i8_scale, &idx->i8_rel_err, &idx->i8_rel_hat, &idx->i8_rowf, &idx->tok_bm, &idx->tok_bm_index}) { b->p = nullptr; b->cap = 0; }
    }
    idx->tok_bm.release(); idx->tok_bm_index.release();
    idx->d_dead.release();
    if (!idx->is_view) { idx->vlong_start.release(); idx->vlong_len.release(); idx->vlong_id.release(); }
    idx->ws_norm_a.release();
    for (DevBuf *b : {&idx->ws_scope_ids, &idx->ws_scope_meta, &idx->ws_scope_bm, &idx->ws_scope_chunks, &idx->ws_scope_sel}) b->release();
    idx->pin_scope.release(); idx->pin_scope_pass.release();
    idx->ws_scope_terms.release(); idx->pin_scope_terms.release();
    for (DevBuf *b : {&idx->ws_near_q, &idx->ws_near_norm, &idx->ws_near_band, &idx->ws_near_cnt, &idx->ws_near_rows}) b->release();
    for (DevBuf *b : {&idx->ws_range_allowed, &idx->ws_range_q, &idx->ws_range_qp, &idx->ws_range_norm, &idx->ws_range_consts, &idx->ws_range_cnt,
                      &idx->ws_range_buf, &idx->ws_range_bdot, &idx->ws_range_list, &idx->ws_range_dots, &idx->ws_range_args}) b->release();
    for (DevBuf *b : {&idx->ws_mask_bm, &idx->ws_mask_chunks, &idx->ws_mask_cnt, &idx->ws_mask_meta}) b->release();
    for (DevBuf *b : {&idx->ws_diverse_pos, &idx->ws_diverse_cnt, &idx->ws_diverse_out, &idx->ws_diverse_gpos, &idx->ws_diverse_gather, &idx->ws_diverse_foreign, &idx->ws_diverse_mask}) b->release();
    idx->pin_diverse.release();
    idx->pin_diverse_rows.release();
    idx->pin_mask.release();
    for (DevBuf *b : {&idx->ws_group_bm, &idx->ws_group_chunks, &idx->ws_group_meta}) b->release();
    idx->pin_group.release();
    DevBuf *bufs[] = {&idx->ws_q, &idx->ws_dot, &idx->ws_dotf, &idx->ws_rowc, &idx->ws_tau, &idx->ws_qsplit, &idx->ws_fcnt,
                      &idx->ws_fbuf, &idx->ws_fqf, &idx->ws_fany, &idx->ws_tsL, &idx->ws_tskey, &idx->ws_qtiled, &idx->ws_fdot, &idx->ws_pbuf, &idx->ws_psel, &idx->ws_q8, &idx->ws_q8s1, &idx->ws_q8err, &idx->ws_zero, &idx->ws_sel, &idx->ws_cand, &idx->ws_qc, &idx->ws_keys_a, &idx->ws_keys_b,
                      &idx->ws_vals_a, &idx->ws_vals_b, &idx->ws_sort_tmp, &idx->ws_raw, &idx->ws_src_start, &idx->ws_qsub,
                      &idx->ws_vmatch, &idx->ws_bitmaps, &idx->ws_hits, &idx->ws_counter, &idx->ws_meta, &idx->ws_tickets, &idx->ws_kwalias};
    for (auto b : bufs) b->release();
    idx->emb_shadow.release();
    idx->emb_i8.release(); idx->i8_scale.release(); idx->i8_rel_err.release(); idx->i8_rel_hat.release(); idx->i8_rowf.release();
    idx->pin_meta.release(); idx->pin_q.release(); idx->pin_qc.release(); idx->pin_cand.release(); idx->pin_norm.release(); idx->pin_cnt.release(); idx->pin_kwcnt.release();
    if (idx->ev_q) (void)hipEventDestroy(idx->ev_q);
    if (idx->stream) (void)hipStreamDestroy(idx->stream);
    delete idx;
}

int orr_index_set_row_base(orr_index *idx, int64_t row_base)
{
    if (!idx || row_base < 0) return fail(ORR_EINVAL, "orr_index_set_row_base: bad argument");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    for_each_lane(idx, [&](orr_index *x) { x->row_base = row_base; });
    return ORR_OK;
}

int64_t orr_index_rows(const orr_index *idx) { return idx ? idx->n_rows : 0; }
int32_t orr_index_dim(const orr_index *idx) { return idx ? idx->dim : 0; }

int orr_index_append(orr_index *idx, int64_t n, int32_t dim, const float *emb, const int64_t *created_ticks,
                     const uint8_t *content_lower, const uint64_t *content_off, const int64_t *row_ids)
{
    if (!idx) return fail(ORR_EINVAL, "orr_index_append: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    if (idx->sealed) return fail(ORR_ESTATE, "orr_index_append: index is sealed");
    if (n < 0) return fail(ORR_EINVAL, "orr_index_append: negative row count");
    if (n == 0) return ORR_OK;
    if (!created_ticks || !content_off) return fail(ORR_EINVAL, "orr_index_append: created_ticks and content_off are required");
    if (dim != 0 && dim != idx->dim)
        return fail(ORR_EDIM, "orr_index_append: dim %d differs from the index dimension %d", dim, idx->dim);
    if (dim != 0 && !emb) return fail(ORR_EINVAL, "orr_index_append: emb is NULL with dim %d", dim);
    if (idx->n_rows + n >= (int64_t)0xFFFFFFFFll) return fail(ORR_EINVAL, "orr_index_append: more than 2^32-1 rows in one shard");
    ORR_TRY(bind_device(idx));
    ORR_TRY(ensure_row_capacity(idx, idx->n_rows + n));

    // content offsets: bring to the host, rebase onto the pool
    std::vector<uint64_t> off((size_t)n + 1);
    HIP_TRY(hipMemcpy(off.data(), content_off, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDefault));
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(ORR_EINVAL, "orr_index_append: content_off is not monotone at row %lld", (long long)i);
    const uint64_t bytes = off[n] - off[0];
    if (bytes > 0 && !content_lower) return fail(ORR_EINVAL, "orr_index_append: content_lower is NULL");
    // re-lay the rows out for the scan kernel: 16-byte aligned starts, space padding behind each row
    std::vector<uint64_t> src_start((size_t)n), dst_start((size_t)n);
    std::vector<uint32_t> lens((size_t)n);
    uint64_t cursor = idx->pool_len;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t len = off[i + 1] - off[i];
        if (len >= (1ull << 31)) return fail(ORR_EINVAL, "orr_index_append: content of row %lld exceeds 2 GiB", (long long)i);
        src_start[i] = off[i] - off[0];
        dst_start[i] = cursor;
        lens[i] = (uint32_t)len;
        cursor += orr::padded_row_bytes(len);
    }
    ORR_TRY(ensure_pool_capacity(idx, cursor));
    HIP_TRY(hipMemsetAsync(idx->d_pool + idx->pool_len, 0x20, cursor - idx->pool_len, idx->stream));
    HIP_TRY(hipMemcpyAsync(idx->d_cstart + idx->n_rows, dst_start.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, idx->stream));
    HIP_TRY(hipMemcpyAsync(idx->d_clen + idx->n_rows, lens.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, idx->stream));
    if (bytes > 0) {
        ORR_TRY(idx->ws_raw.reserve(bytes));
        ORR_TRY(idx->ws_src_start.reserve(sizeof(uint64_t) * (size_t)n));
        HIP_TRY(hipMemcpyAsync(idx->ws_raw.p, content_lower + off[0], bytes, hipMemcpyDefault, idx->stream));
        HIP_TRY(hipMemcpyAsync(idx->ws_src_start.p, src_start.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, idx->stream));
        HIP_TRY(orr::launch_gather_content(idx->ws_raw.as<uint8_t>(), idx->ws_src_start.as<uint64_t>(), idx->d_clen + idx->n_rows,
                                           idx->d_pool, idx->d_cstart + idx->n_rows, nullptr, n, idx->stream));
    }
    HIP_TRY(hipStreamSynchronize(idx->stream));

    // timestamps (host mirror + device)
    const size_t old = idx->h_created.size();
    idx->h_created.resize(old + (size_t)n);
    HIP_TRY(hipMemcpy(idx->h_created.data() + old, created_ticks, sizeof(int64_t) * (size_t)n, hipMemcpyDefault));
    HIP_TRY(hipMemcpyAsync(idx->d_created + idx->n_rows, idx->h_created.data() + old, sizeof(int64_t) * (size_t)n,
                           hipMemcpyHostToDevice, idx->stream));

    // embeddings: copy, or zero rows (a zero row has normB = 0 -> cosine 0, the same
    // value the null/empty guard of RecallSearchService.cs:71 yields)
    if (idx->dim > 0) {
        float *dst = idx->d_emb + (size_t)idx->n_rows * idx->dim;
        const size_t eb = sizeof(float) * (size_t)n * idx->dim;
        if (dim == idx->dim)
            HIP_TRY(hipMemcpyAsync(dst, emb, eb, hipMemcpyDefault, idx->stream));
        else
            HIP_TRY(hipMemsetAsync(dst, 0, eb, idx->stream));
    }
    if (row_ids)
        HIP_TRY(hipMemcpyAsync(idx->d_row_ids + idx->n_rows, row_ids, sizeof(int64_t) * (size_t)n, hipMemcpyDefault, idx->stream));
    else
        HIP_TRY(orr::launch_iota_i64(idx->d_row_ids + idx->n_rows, n, idx->row_base + idx->n_rows, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    idx->h_clen.insert(idx->h_clen.end(), lens.begin(), lens.end());
    idx->pool_len = cursor;
    idx->n_rows += n;
    return ORR_OK;
}

int orr_index_seal(orr_index *idx)
{
    if (!idx) return fail(ORR_EINVAL, "orr_index_seal: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    if (idx->sealed) return ORR_OK;
    ORR_TRY(bind_device(idx));
    const int64_t n = idx->n_rows;

    // candidate order: stable sort by CreatedAt descending (InMemoryIngestionStore.cs:61)
    std::vector<int64_t> perm((size_t)n);
    std::iota(perm.begin(), perm.end(), (int64_t)0);
    const int64_t *cr = idx->h_created.data();
    bool identity = true;
    for (int64_t i = 1; i < n && identity; ++i) identity = cr[i - 1] >= cr[i];
    if (!identity) {
        std::stable_sort(perm.begin(), perm.end(), [cr](int64_t a, int64_t b) { return cr[a] > cr[b]; });
        int64_t *d_perm = nullptr;
        ORR_TRY(dev_alloc(&d_perm, (size_t)n));
        HIP_TRY(hipMemcpyAsync(d_perm, perm.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, idx->stream));
        if (idx->dim > 0) {
            float *ne = nullptr;
            ORR_TRY(dev_alloc(&ne, (size_t)idx->cap_rows * idx->dim));
            HIP_TRY(orr::launch_gather_rows_f32(idx->d_emb, ne, d_perm, n, idx->dim, idx->stream));
            HIP_TRY(hipStreamSynchronize(idx->stream));
            (void)hipFree(idx->d_emb);
            idx->d_emb = ne;
        }
        int64_t *nc = nullptr, *nr = nullptr;
        ORR_TRY(dev_alloc(&nc, (size_t)idx->cap_rows));
        ORR_TRY(dev_alloc(&nr, (size_t)idx->cap_rows));
        HIP_TRY(orr::launch_gather_i64(idx->d_created, nc, d_perm, n, idx->stream));
        HIP_TRY(orr::launch_gather_i64(idx->d_row_ids, nr, d_perm, n, idx->stream));
        std::vector<uint64_t> nstart((size_t)n);
        std::vector<uint32_t> nlen((size_t)n);
        uint64_t cursor = 0;
        for (int64_t p = 0; p < n; ++p) {
            nlen[p] = idx->h_clen[perm[p]];
            nstart[p] = cursor;
            cursor += orr::padded_row_bytes(nlen[p]);
        }
        uint64_t *d_nstart = nullptr;
        uint32_t *d_nlen = nullptr;
        uint8_t *npool = nullptr;
        ORR_TRY(dev_alloc(&d_nstart, (size_t)idx->cap_rows));
        ORR_TRY(dev_alloc(&d_nlen, (size_t)idx->cap_rows));
        ORR_TRY(dev_alloc(&npool, (size_t)idx->pool_cap));
        HIP_TRY(hipMemsetAsync(npool, 0x20, cursor, idx->stream));
        HIP_TRY(hipMemcpyAsync(d_nstart, nstart.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, idx->stream));
        HIP_TRY(orr::launch_gather_content(idx->d_pool, idx->d_cstart, idx->d_clen, npool, d_nstart, d_perm, n, idx->stream));
        HIP_TRY(orr::launch_gather_u32(idx->d_clen, d_nlen, d_perm, n, idx->stream));
        HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(idx->d_created); idx->d_created = nc;
        (void)hipFree(idx->d_row_ids); idx->d_row_ids = nr;
        (void)hipFree(idx->d_cstart); idx->d_cstart = d_nstart;
        (void)hipFree(idx->d_clen); idx->d_clen = d_nlen;
        (void)hipFree(idx->d_pool); idx->d_pool = npool;
        idx->pool_len = cursor;
        (void)hipFree(d_perm);
        std::vector<int64_t> sorted_created((size_t)n);
        for (int64_t p = 0; p < n; ++p) sorted_created[p] = cr[perm[p]];
        idx->h_created.swap(sorted_created);
        idx->h_clen.swap(nlen);
    }
    idx->h_cprefix.assign((size_t)n + 1, 0);
    for (int64_t p = 0; p < n; ++p) idx->h_cprefix[p + 1] = idx->h_cprefix[p] + idx->h_clen[p];

    // token index: content goes to the host once, comes back as vocabulary + postings,
    // and the raw text leaves HBM
    if (n > 0) {
        std::vector<uint8_t> h_pool((size_t)idx->pool_len + 16);
        std::vector<uint64_t> h_cstart((size_t)n);
        if (idx->pool_len) HIP_TRY(hipMemcpy(h_pool.data(), idx->d_pool, (size_t)idx->pool_len, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_cstart.data(), idx->d_cstart, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
        orr::TokenIndexHost ti;
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        orr::build_token_index(h_pool.data(), h_cstart.data(), idx->h_clen.data(), n, (int)std::min(hw, 32u), ti);
        idx->n_tokens = (int64_t)ti.vstart.size();
        idx->n_postings = ti.post_rows.size();
        ORR_TRY(dev_alloc(&idx->d_vpool, ti.vpool.size() + orr::kScanPoolSlack));
        ORR_TRY(dev_alloc(&idx->d_vstart, ti.vstart.size()));
        ORR_TRY(dev_alloc(&idx->d_vlen, ti.vlen.size()));
        ORR_TRY(dev_alloc(&idx->d_post_off, ti.post_off.size()));
        ORR_TRY(dev_alloc(&idx->d_post_rows, ti.post_rows.size()));
        HIP_TRY(hipMemsetAsync(idx->d_vpool, 0x20, ti.vpool.size() + orr::kScanPoolSlack, idx->stream));
        if (!ti.vpool.empty()) HIP_TRY(hipMemcpyAsync(idx->d_vpool, ti.vpool.data(), ti.vpool.size(), hipMemcpyHostToDevice, idx->stream));
        if (idx->n_tokens) {
            HIP_TRY(hipMemcpyAsync(idx->d_vstart, ti.vstart.data(), sizeof(uint64_t) * ti.vstart.size(), hipMemcpyHostToDevice, idx->stream));
            HIP_TRY(hipMemcpyAsync(idx->d_vlen, ti.vlen.data(), sizeof(uint32_t) * ti.vlen.size(), hipMemcpyHostToDevice, idx->stream));
        }
        HIP_TRY(hipMemcpyAsync(idx->d_post_off, ti.post_off.data(), sizeof(uint64_t) * ti.post_off.size(), hipMemcpyHostToDevice, idx->stream));
        if (idx->n_postings)
            HIP_TRY(hipMemcpyAsync(idx->d_post_rows, ti.post_rows.data(), sizeof(uint32_t) * ti.post_rows.size(), hipMemcpyHostToDevice, idx->stream));
        HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(idx->d_pool); idx->d_pool = nullptr; idx->pool_cap = 0;
        (void)hipFree(idx->d_cstart); idx->d_cstart = nullptr;
        (void)hipFree(idx->d_clen); idx->d_clen = nullptr;
    }

    // K0: exact row norms, sum_i (double)fl32(e_i*e_i) (RecallSearchService.cs:81)
    ORR_TRY(dev_alloc(&idx->d_norm_b, (size_t)std::max<int64_t>(n, 1)));
    if (idx->dim > 0 && n > 0) {
        Timed t(idx, "row_norms_exact", 4.0 * (double)n * idx->dim + 8.0 * (double)n);
        HIP_TRY(orr::launch_dot_exact(idx->d_emb, n, idx->dim, nullptr, 1, true, idx->d_norm_b, n, idx->stream));
    } else if (n > 0) {
        HIP_TRY(hipMemsetAsync(idx->d_norm_b, 0, sizeof(double) * (size_t)n, idx->stream));
    }
    HIP_TRY(hipStreamSynchronize(idx->stream));
    collect_events(idx);
    idx->sealed = true;
    return ORR_OK;
}

namespace {

struct ShardHeader {
    char magic[8];               // "ORRSHD1\0"
    uint32_t version, dim;
    int64_t n_rows, n_tokens;
    uint64_t n_postings, vpool_bytes;
    uint64_t reserved[4];
};
constexpr size_t kIoChunk = 64u << 20;

int write_device_array(FILE *f, const void *dptr, size_t bytes, std::vector<uint8_t> &buf)
{
    const uint8_t *p = static_cast<const uint8_t *>(dptr);
    for (size_t off = 0; off < bytes; off += kIoChunk) {
        const size_t m = std::min(kIoChunk, bytes - off);
        HIP_TRY(hipMemcpy(buf.data(), p + off, m, hipMemcpyDeviceToHost));
        if (fwrite(buf.data(), 1, m, f) != m) return fail(ORR_EINVAL, "short write to the shard file");
    }
    return ORR_OK;
}

int read_device_array(FILE *f, void *dptr, size_t bytes, std::vector<uint8_t> &buf)
{
    uint8_t *p = static_cast<uint8_t *>(dptr);
    for (size_t off = 0; off < bytes; off += kIoChunk) {
        const size_t m = std::min(kIoChunk, bytes - off);
        if (fread(buf.data(), 1, m, f) != m) return fail(ORR_EINVAL, "shard file is truncated");
        HIP_TRY(hipMemcpy(p + off, buf.data(), m, hipMemcpyHostToDevice));
    }
    return ORR_OK;
}

}  // namespace

int orr_index_save(orr_index *idx, const char *path)
{
    if (!idx || !path) return fail(ORR_EINVAL, "orr_index_save: null argument");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_save: index is not sealed");
    if (idx->is_view) return fail(ORR_ESTATE, "orr_index_save: save the owning index, not a view");
    ORR_TRY(bind_device(idx));
    FILE *f = fopen(path, "wb");
    if (!f) return fail(ORR_EINVAL, "orr_index_save: cannot open %s", path);
    ShardHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "ORRSHD1", 8);
    h.version = 1; h.dim = (uint32_t)idx->dim; h.n_rows = idx->n_rows; h.n_tokens = idx->n_tokens;
    h.n_postings = idx->n_postings;
    h.reserved[0] = (uint64_t)idx->dead.size();          // deleted positions follow the last array
    uint64_t vpool_bytes = 0;
    std::vector<uint64_t> vstart((size_t)idx->n_tokens);
    std::vector<uint32_t> vlen((size_t)idx->n_tokens);
    if (idx->n_tokens > 0) {
        hipError_t e1 = hipMemcpy(vstart.data(), idx->d_vstart, sizeof(uint64_t) * vstart.size(), hipMemcpyDeviceToHost);
        hipError_t e2 = hipMemcpy(vlen.data(), idx->d_vlen, sizeof(uint32_t) * vlen.size(), hipMemcpyDeviceToHost);
        if (e1 != hipSuccess || e2 != hipSuccess) { fclose(f); return fail(ORR_EDEVICE, "orr_index_save: device copy failed"); }
        vpool_bytes = vstart.back() + orr::padded_row_bytes(vlen.back());
    }
    h.vpool_bytes = vpool_bytes;
    std::vector<uint8_t> buf(kIoChunk);
    const size_t n = (size_t)idx->n_rows, V = (size_t)idx->n_tokens;
    int r = fwrite(&h, sizeof(h), 1, f) == 1 ? ORR_OK : fail(ORR_EINVAL, "short write to the shard file");
    if (r == ORR_OK && idx->dim > 0) r = write_device_array(f, idx->d_emb, sizeof(float) * n * idx->dim, buf);
    if (r == ORR_OK) r = write_device_array(f, idx->d_norm_b, sizeof(double) * n, buf);
    if (r == ORR_OK) r = write_device_array(f, idx->d_created, sizeof(int64_t) * n, buf);
    if (r == ORR_OK) r = write_device_array(f, idx->d_row_ids, sizeof(int64_t) * n, buf);
    if (r == ORR_OK && n) r = fwrite(idx->h_clen.data(), sizeof(uint32_t), n, f) == n ? ORR_OK : fail(ORR_EINVAL, "short write");
    if (r == ORR_OK && V) {
        r = fwrite(vstart.data(), sizeof(uint64_t), V, f) == V && fwrite(vlen.data(), sizeof(uint32_t), V, f) == V
                ? ORR_OK : fail(ORR_EINVAL, "short write");
        if (r == ORR_OK) r = write_device_array(f, idx->d_vpool, vpool_bytes, buf);
    }
    if (r == ORR_OK && n) r = write_device_array(f, idx->d_post_off, sizeof(uint64_t) * (V + 1), buf);
    if (r == ORR_OK && idx->n_postings) r = write_device_array(f, idx->d_post_rows, sizeof(uint32_t) * (size_t)idx->n_postings, buf);
    if (r == ORR_OK && !idx->dead.empty())
        r = fwrite(idx->dead.data(), sizeof(int64_t), idx->dead.size(), f) == idx->dead.size() ? ORR_OK : fail(ORR_EINVAL, "short write");
    if (fclose(f) != 0 && r == ORR_OK) r = fail(ORR_EINVAL, "orr_index_save: close failed");
    return r;
}

int orr_index_load(const orr_config *cfg, const char *path, orr_index **out)
{
    if (!cfg || !path || !out) return fail(ORR_EINVAL, "orr_index_load: null argument");
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(ORR_EINVAL, "orr_index_load: cannot open %s", path);
    ShardHeader h;
    if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "ORRSHD1", 8) != 0 || h.version != 1 || h.n_rows < 0 || h.n_tokens < 0) {
        fclose(f);
        return fail(ORR_EINVAL, "orr_index_load: %s is not a version-1 shard file", path);
    }
    if (cfg->dim != 0 && cfg->dim != (int32_t)h.dim) {
        fclose(f);
        return fail(ORR_EDIM, "orr_index_load: file dimension %u differs from the requested %d", h.dim, cfg->dim);
    }
    {   // the header's counts against the size of the file, before anything is allocated from them
        long at = ftell(f), end = -1;
        if (at >= 0 && fseek(f, 0, SEEK_END) == 0) end = ftell(f);
        if (at < 0 || end < 0 || fseek(f, at, SEEK_SET) != 0) { fclose(f); return fail(ORR_EINVAL, "orr_index_load: cannot size %s", path); }
        const long double nn = (long double)h.n_rows, vv = (long double)h.n_tokens;
        long double want = (long double)sizeof(h) + nn * (4.0L * h.dim + 8 + 8 + 8 + 4) + (long double)h.n_postings * 4 + (long double)h.reserved[0] * 8;
        if (h.n_tokens) want += vv * 12 + (long double)h.vpool_bytes;
        if (h.n_rows) want += (vv + 1) * 8;
        if (want != (long double)end) {
            fclose(f);
            return fail(ORR_EINVAL, "orr_index_load: %s: the header's counts do not add up to the file's size", path);
        }
    }
    orr_config c = *cfg;
    c.dim = (int32_t)h.dim;
    c.capacity_rows = h.n_rows;
    orr_index *idx = nullptr;
    int r = orr_index_create(&c, &idx);
    if (r != ORR_OK) { fclose(f); return r; }
    // idx is private to this call until it is returned: no locking needed
    const size_t n = (size_t)h.n_rows, V = (size_t)h.n_tokens;
    std::vector<uint8_t> buf(kIoChunk);
    idx->n_rows = h.n_rows; idx->n_tokens = h.n_tokens; idx->n_postings = h.n_postings;
    auto body = [&]() -> int {
        if (idx->dim > 0) ORR_TRY(read_device_array(f, idx->d_emb, sizeof(float) * n * idx->dim, buf));
        ORR_TRY(dev_alloc(&idx->d_norm_b, std::max<size_t>(n, 1)));
        ORR_TRY(read_device_array(f, idx->d_norm_b, sizeof(double) * n, buf));
        idx->h_created.resize(n);
        const long pos = ftell(f);
        if (n && fread(idx->h_created.data(), sizeof(int64_t), n, f) != n) return fail(ORR_EINVAL, "shard file is truncated");
        fseek(f, pos, SEEK_SET);
        ORR_TRY(read_device_array(f, idx->d_created, sizeof(int64_t) * n, buf));
        ORR_TRY(read_device_array(f, idx->d_row_ids, sizeof(int64_t) * n, buf));
        idx->h_clen.resize(n);
        if (n && fread(idx->h_clen.data(), sizeof(uint32_t), n, f) != n) return fail(ORR_EINVAL, "shard file is truncated");
        idx->h_cprefix.assign(n + 1, 0);
        for (size_t p = 0; p < n; ++p) idx->h_cprefix[p + 1] = idx->h_cprefix[p] + idx->h_clen[p];
        if (V) {
            ORR_TRY(dev_alloc(&idx->d_vstart, V));
            ORR_TRY(dev_alloc(&idx->d_vlen, V));
            ORR_TRY(dev_alloc(&idx->d_vpool, (size_t)h.vpool_bytes + orr::kScanPoolSlack));
            std::vector<uint64_t> vstart_h(V);
            ORR_TRY(read_device_array_checked(f, idx->d_vstart, V, buf, [&](const uint64_t *x, size_t off, size_t m) {
                for (size_t i = 0; i < m; ++i) { if (x[i] > h.vpool_bytes) return false; vstart_h[off + i] = x[i]; }
                return true; }, "vocabulary offsets"));
            ORR_TRY(read_device_array_checked(f, idx->d_vlen, V, buf, [&](const uint32_t *x, size_t off, size_t m) {
                for (size_t i = 0; i < m; ++i) if (vstart_h[off + i] + orr::padded_row_bytes(x[i]) > h.vpool_bytes) return false;
                return true; }, "vocabulary lengths"));
            HIP_TRY(hipMemset(idx->d_vpool, 0x20, (size_t)h.vpool_bytes + orr::kScanPoolSlack));
            ORR_TRY(read_device_array(f, idx->d_vpool, (size_t)h.vpool_bytes, buf));
        }
        if (n) {
            ORR_TRY(dev_alloc(&idx->d_post_off, V + 1));
            uint64_t prev = 0;
            ORR_TRY(read_device_array_checked(f, idx->d_post_off, V + 1, buf, [&](const uint64_t *x, size_t off, size_t m) {
                for (size_t i = 0; i < m; ++i) {
                    if (x[i] < prev || x[i] > h.n_postings || (off + i == 0 && x[i] != 0) || (off + i == V && x[i] != h.n_postings)) return false;
                    prev = x[i];
                }
                return true; }, "posting offsets"));
        } else if (h.n_postings) {
            return fail(ORR_EINVAL, "shard file: postings without rows");
        }
        ORR_TRY(dev_alloc(&idx->d_post_rows, std::max<size_t>((size_t)h.n_postings, 1)));
        if (h.n_postings)
            ORR_TRY(read_device_array_checked(f, idx->d_post_rows, (size_t)h.n_postings, buf, [&](const uint32_t *x, size_t, size_t m) {
                for (size_t i = 0; i < m; ++i) if ((uint64_t)x[i] >= (uint64_t)n) return false;
                return true; }, "posting rows"));
        if (h.reserved[0]) {                          // deleted rows: norms and timestamps in the file are already overwritten
            if (h.reserved[0] > (uint64_t)n) return fail(ORR_EINVAL, "shard file lists more deleted rows than rows");
            idx->dead.resize((size_t)h.reserved[0]);
            if (fread(idx->dead.data(), sizeof(int64_t), idx->dead.size(), f) != idx->dead.size()) return fail(ORR_EINVAL, "shard file is truncated");
            for (size_t i = 0; i < idx->dead.size(); ++i)
                if (idx->dead[i] < 0 || idx->dead[i] >= (int64_t)n || (i && idx->dead[i] <= idx->dead[i - 1]))
                    return fail(ORR_EINVAL, "shard file has a malformed deleted-row list");
            ORR_TRY(idx->d_dead.reserve(sizeof(int64_t) * idx->dead.size()));
            HIP_TRY(hipMemcpy(idx->d_dead.p, idx->dead.data(), sizeof(int64_t) * idx->dead.size(), hipMemcpyHostToDevice));
            idx->lanes.update_shared([&](LanePool::Shared &sh) { sh.dead_count = (int64_t)idx->dead.size(); });
            // the host mirror must stay a descending sequence (orr_index_insert_rows plans on it, a cluster compares its ends)
            orr::repair_dead_ticks(idx->h_created, idx->dead);
        }
        return ORR_OK;
    };
    r = body();
    fclose(f);
    if (r != ORR_OK) {
        const std::string keep = g_last_error;
        orr_index_destroy(idx);
        g_last_error = keep;
        return r;
    }
    // the raw content buffers of an unsealed index are not part of a shard file
    if (idx->d_cstart) { (void)hipFree(idx->d_cstart); idx->d_cstart = nullptr; }
    if (idx->d_clen) { (void)hipFree(idx->d_clen); idx->d_clen = nullptr; }
    idx->sealed = true;
    *out = idx;
    return ORR_OK;
}

// bf16 shadow of the sealed embeddings for the screening GEMM.  Half the master's bytes; when the
// allocation does not fit, the two-stage pass converts in the kernel instead (orr_gemm.hip, PROD = 1).
static int ensure_shadow(orr_index *idx)
{
    if (idx->is_view) return ORR_OK;                   // taken from the parent at creation, or absent
    if (idx->shadow_ready || idx->shadow_failed || !idx->sealed || idx->n_rows <= 0 || idx->dim <= 0 || idx->dim % 64 != 0) return ORR_OK;
    const size_t bytes = orr::bf16_tiled_bytes(idx->n_rows, idx->dim);
    size_t free_b = 0, total_b = 0;
    // (a buffer that already holds the bytes -- the rebuild behind orr_index_insert_rows -- needs no new room)
    if (idx->emb_shadow.cap < bytes && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + bytes / 8 + ((size_t)4 << 30))) {   // keep 4 GiB for workspaces
        idx->shadow_failed = true;
        return ORR_OK;
    }
    if (idx->emb_shadow.reserve(bytes) != ORR_OK) {
        (void)hipGetLastError();
        idx->shadow_failed = true;
        return ORR_OK;
    }
    HIP_TRY(orr::launch_bf16_tiled(idx->d_emb, idx->n_rows, idx->dim, idx->emb_shadow.p, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    idx->shadow_ready = true;
    return ORR_OK;
}

// Int8 shadow (a quarter of the master's bytes): operand of the streaming screen of 1..4 queries (K2i) and of
// the screening GEMM of larger batches (K2j).  Where it exists the bf16 shadow is only built for what it
// does not cover (5..8 queries, dimensions that are not a multiple of 128).
static int ensure_i8_shadow(orr_index *idx)
{
    if (idx->is_view || idx->i8_ready || idx->i8_failed || !idx->sealed || idx->n_rows <= 0 || idx->dim <= 0 || idx->dim % 128 != 0) return ORR_OK;
    const size_t bytes = orr::i8_tiled_bytes(idx->n_rows, idx->dim) + 28 * (size_t)idx->n_rows;
    size_t free_b = 0, total_b = 0;
    if (idx->emb_i8.cap < orr::i8_tiled_bytes(idx->n_rows, idx->dim) &&
        (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + bytes / 8 + ((size_t)8 << 30))) {   // keep 8 GiB for workspaces
        idx->i8_failed = true;
        return ORR_OK;
    }
    if (idx->emb_i8.reserve(orr::i8_tiled_bytes(idx->n_rows, idx->dim)) != ORR_OK || idx->i8_scale.reserve(sizeof(float) * (size_t)idx->n_rows) != ORR_OK ||
        idx->i8_rel_err.reserve(sizeof(float) * (size_t)idx->n_rows) != ORR_OK ||
        idx->i8_rel_hat.reserve(sizeof(float) * (size_t)idx->n_rows) != ORR_OK ||
        idx->i8_rowf.reserve(sizeof(float4) * (size_t)idx->n_rows) != ORR_OK) {
        (void)hipGetLastError();
        idx->emb_i8.release(); idx->i8_scale.release(); idx->i8_rel_err.release(); idx->i8_rel_hat.release(); idx->i8_rowf.release();
        idx->i8_failed = true;
        return ORR_OK;
    }
    HIP_TRY(orr::launch_i8_shadow(idx->d_emb, idx->d_norm_b, idx->n_rows, idx->dim, idx->emb_i8.p, idx->i8_scale.as<float>(),
                                  idx->i8_rel_err.as<float>(), idx->i8_rel_hat.as<float>(), idx->stream));
    HIP_TRY(orr::launch_i8_rowf(idx->i8_scale.as<float>(), idx->i8_rel_err.as<float>(), idx->i8_rel_hat.as<float>(), idx->n_rows,
                                idx->i8_rowf.as<float4>(), idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    idx->i8_ready = true;
    return ORR_OK;
}

// The long tokens of the vocabulary as their own row list for the wave-per-token scan.
static int ensure_vlong(orr_index *idx)
{
    if (idx->n_vlong >= 0 || idx->is_view) return ORR_OK;          // a view copies its parent's at creation
    const size_t V = (size_t)idx->n_tokens;
    std::vector<uint64_t> start, vstart(V);
    std::vector<uint32_t> len, id, vlen(V);
    if (V) {
        HIP_TRY(hipMemcpy(vstart.data(), idx->d_vstart, sizeof(uint64_t) * V, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(vlen.data(), idx->d_vlen, sizeof(uint32_t) * V, hipMemcpyDeviceToHost));
    }
    for (int pass = 0; pass < 2; ++pass) {                         // 17..32 bytes first, the longer ones behind them
        for (size_t v = 0; v < V; ++v)
            if (vlen[v] > 16 && (vlen[v] <= 32) == (pass == 0)) { start.push_back(vstart[v]); len.push_back(vlen[v]); id.push_back((uint32_t)v); }
        if (pass == 0) idx->n_vmid = (int64_t)id.size();
    }
    if (!id.empty()) {
        ORR_TRY(idx->vlong_start.reserve(sizeof(uint64_t) * id.size()));
        ORR_TRY(idx->vlong_len.reserve(sizeof(uint32_t) * id.size()));
        ORR_TRY(idx->vlong_id.reserve(sizeof(uint32_t) * id.size()));
        HIP_TRY(hipMemcpy(idx->vlong_start.p, start.data(), sizeof(uint64_t) * id.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(idx->vlong_len.p, len.data(), sizeof(uint32_t) * id.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(idx->vlong_id.p, id.data(), sizeof(uint32_t) * id.size(), hipMemcpyHostToDevice));
    }
    idx->n_vlong = (int64_t)id.size();
    return ORR_OK;
}

// Row bitmaps of the frequent vocabulary tokens (see orr_index::tok_bm), through the same posting expansion a batch runs.
static int ensure_token_bitmaps(orr_index *idx)
{
    if (idx->is_view || idx->n_tok_bm >= 0 || !idx->sealed) return ORR_OK;    // a view copies its parent's at creation
    idx->n_tok_bm = 0;
    if (const char *e = getenv("ORR_TOKEN_BITMAPS")) { if (atoi(e) == 0) return ORR_OK; }      // diagnostic: A/B against per-batch expansion
    const int64_t n = idx->n_rows, V = idx->n_tokens;
    if (n < 48 * (int64_t)orr::kSelSegRows || V <= 0 || idx->n_postings == 0) return ORR_OK;   // small shards expand in microseconds
    const int64_t words = keyword::words_per_term(n);
    std::vector<uint64_t> off((size_t)V + 1);
    HIP_TRY(hipMemcpy(off.data(), idx->d_post_off, sizeof(uint64_t) * ((size_t)V + 1), hipMemcpyDeviceToHost));
    std::vector<uint32_t> toks;
    for (int64_t v = 0; v < V; ++v)
        if ((off[(size_t)v + 1] - off[(size_t)v]) * 64 >= (uint64_t)n) toks.push_back((uint32_t)v);
    if (toks.empty()) return ORR_OK;
    const size_t bytes = toks.size() * (size_t)words * sizeof(uint32_t);
    size_t free_b = 0, total_b = 0;
    if (bytes > ((size_t)32 << 30) || hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + ((size_t)12 << 30)) return ORR_OK;   // no room: expand per batch
    if (idx->tok_bm.reserve(bytes) != ORR_OK || idx->tok_bm_index.reserve(sizeof(int32_t) * (size_t)V) != ORR_OK) {
        (void)hipGetLastError();
        idx->tok_bm.release(); idx->tok_bm_index.release();
        return ORR_OK;
    }
    std::vector<int32_t> index((size_t)V, -1);
    std::vector<orr::KwHit> hits(toks.size());
    uint64_t chunks = 0;
    for (size_t j = 0; j < toks.size(); ++j) {
        const uint32_t v = toks[j];
        index[v] = (int32_t)j;
        orr::KwHit h;
        h.post_begin = off[v]; h.post_len = (uint32_t)(off[(size_t)v + 1] - off[v]); h.chunk_base = (uint32_t)chunks; h.term = (uint32_t)j; h.token = v;
        hits[j] = h;
        chunks += (h.post_len + orr::kPostChunk - 1) / orr::kPostChunk;
    }
    if (chunks >= ((uint64_t)1 << 32)) { idx->tok_bm.release(); idx->tok_bm_index.release(); return ORR_OK; }
    const unsigned long long counter = ((unsigned long long)toks.size() << 32) | (unsigned long long)chunks;
    DevBuf d_hits, d_counter;
    ORR_TRY(d_hits.reserve(sizeof(orr::KwHit) * hits.size()));
    ORR_TRY(d_counter.reserve(sizeof(counter)));
    hipStream_t s = idx->stream;
    hipError_t e = hipMemcpyAsync(d_hits.p, hits.data(), sizeof(orr::KwHit) * hits.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_counter.p, &counter, sizeof(counter), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(idx->tok_bm_index.p, index.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(idx->tok_bm.p, 0, bytes, s);
    if (e == hipSuccess) e = orr::launch_expand_hits(d_hits.as<orr::KwHit>(), d_counter.as<unsigned long long>(), (uint32_t)hits.size(), idx->d_post_rows,
                                                     idx->tok_bm.as<uint32_t>(), words, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    d_hits.release(); d_counter.release();
    if (e != hipSuccess) {
        idx->tok_bm.release(); idx->tok_bm_index.release();
        return fail(ORR_EDEVICE, "token bitmaps: %s", hipGetErrorString(e));
    }
    idx->n_tok_bm = (int64_t)toks.size();
    idx->tok_bm_words = words;
    return ORR_OK;
}

int64_t orr_index_live_rows(const orr_index *idx)
{
    return idx ? idx->n_rows - (int64_t)(idx->parent ? idx->parent->dead.size() : idx->dead.size()) : 0;
}

// The id table of scoped searches goes when positions move (the caller holds Exclusive: no search reads it).
// `held` is the caller's lock on the index's scope_mu (ScopeRemap takes it for the whole move): ensure_scope_table builds the
// table under that mutex.
static void drop_scope_table(orr_index *idx, const std::unique_lock<std::mutex> &held)
{
    if (!held.owns_lock() || held.mutex() != &idx->scope_mu) {
        fprintf(stderr, "omnirecall: drop_scope_table without the index's scope_mu held\n");
        abort();
    }
    if (idx->scope_tab_ids) (void)hipFree(idx->scope_tab_ids);
    if (idx->scope_tab_pos) (void)hipFree(idx->scope_tab_pos);
    idx->scope_tab_ids = nullptr; idx->scope_tab_pos = nullptr;
    idx->scope_ready.store(false, std::memory_order_release);
}

// The live rows (not deleted) that carry the ids want[0..n): (position, index into want) for each, in the order of `want`;
// a duplicate id of orr_index_append gives several.  Ids map to positions through idx->id_index, built at the first call.
static int live_rows_of_ids(orr_index *idx, const std::vector<int64_t> &want, std::vector<std::pair<int64_t, int64_t>> &out)
{
    const size_t rows = (size_t)idx->n_rows;
    if (idx->id_index.empty()) {                       // ids -> positions, once
        std::vector<int64_t> ids(rows);
        HIP_TRY(hipMemcpy(ids.data(), idx->d_row_ids, sizeof(int64_t) * rows, hipMemcpyDeviceToHost));
        idx->id_index.resize(rows);
        for (size_t p = 0; p < rows; ++p) idx->id_index[p] = {ids[p], (int64_t)p};
        std::sort(idx->id_index.begin(), idx->id_index.end());
    }
    out.clear();
    for (size_t i = 0; i < want.size(); ++i) {
        auto it = std::lower_bound(idx->id_index.begin(), idx->id_index.end(), std::make_pair(want[i], (int64_t)-1));
        for (; it != idx->id_index.end() && it->first == want[i]; ++it)
            if (!std::binary_search(idx->dead.begin(), idx->dead.end(), it->second)) out.push_back({it->second, (int64_t)i});
    }
    return ORR_OK;
}

// ---- scope handles through maintenance (orr_scope; the rules are orr_scope_set_plan.h's) -------------------------------------

static void free_scope_arrays(uint32_t *bm, uint32_t *chunks)
{
    if (bm) (void)hipFree(bm);
    if (chunks) (void)hipFree(chunks);
}

// The bitmap and the chunk counts of a scope over `rows` rows (neither is initialised).
static int alloc_scope_arrays(int64_t rows, uint32_t **bm, uint32_t **chunks, int64_t *words)
{
    *words = (int64_t)(scope::bitmap_bytes(rows) / 4);
    *bm = nullptr; *chunks = nullptr;
    int r = dev_alloc(bm, (size_t)*words);
    if (r == ORR_OK) r = dev_alloc(chunks, (size_t)orr::scope_chunks(*words));
    if (r != ORR_OK) { (void)hipGetLastError(); free_scope_arrays(*bm, *chunks); *bm = nullptr; *chunks = nullptr; }
    return r;
}

// What a scope keeps beside its bitmap, brought up to date after the bitmap changed: the chunk counts, live, n_clip_all (as
// mask_clip with took = live: the live-th set bit is the last one).  On the lane the caller holds; ends synchronised.
static int refresh_scope(orr_index *lane, orr_scope *sc)
{
    hipStream_t s = lane->stream;
    ORR_TRY(lane->pin_scope.reserve(16));              // [limit i64][live u32][took u32]
    ORR_TRY(lane->ws_scope_meta.reserve(8));
    ORR_TRY(lane->pin_mask.reserve(sizeof(int64_t)));
    uint8_t *hp = lane->pin_scope.as<uint8_t>();
    *reinterpret_cast<int64_t *>(hp) = std::numeric_limits<int64_t>::max();
    uint32_t *h_live = reinterpret_cast<uint32_t *>(hp + 8);
    HIP_TRY(hipMemcpyAsync(lane->ws_scope_meta.p, hp, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(orr::launch_scope_counts(sc->bm, sc->words, 1, 1, lane->ws_scope_meta.as<int64_t>(), sc->chunks, h_live, h_live + 1, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t live = (int64_t)*h_live;
    int64_t clip = 0;
    if (live > 0) {
        HIP_TRY(orr::launch_mask_clip(sc->bm, sc->words, sc->chunks, (uint32_t)live, lane->pin_mask.as<int64_t>(), s));
        HIP_TRY(hipStreamSynchronize(s));
        clip = std::min<int64_t>(*lane->pin_mask.as<int64_t>(), sc->n_rows);
    }
    collect_events(lane);
    sc->n_clip_all = clip;
    sc->live.store(live);
    return ORR_OK;
}

// A scope loses its device memory and its shard: every later call on it is ORR_ESTATE (the caller holds sc->mu exclusively and
// takes it out of the index's list).
static void orphan_scope(orr_scope *sc)
{
    free_scope_arrays(sc->bm, sc->chunks);
    sc->bm = nullptr; sc->chunks = nullptr;
    sc->live.store(-1);
    sc->owner.store(nullptr);
}

// Every scope of idx->scopes through change(scope) and refresh_scope.  A scope whose bitmap changed but whose counts could not
// be brought up to date (a device error) must not be searched with stale counts: it is orphaned, and the first error returned.
// The caller holds scope_mu.
static int change_scopes(orr_index *idx, const std::function<int(size_t, orr_scope *)> &change)
{
    int r = ORR_OK;
    std::vector<orr_scope *> kept;
    for (size_t i = 0; i < idx->scopes.size(); ++i) {
        orr_scope *sc = idx->scopes[i];
        std::unique_lock<std::shared_mutex> w(sc->mu);
        int ri = change(i, sc);
        if (ri == ORR_OK) ri = refresh_scope(idx, sc);
        if (ri == ORR_OK) { kept.push_back(sc); continue; }
        (void)hipStreamSynchronize(idx->stream);
        (void)hipGetLastError();
        orphan_scope(sc);
        if (r == ORR_OK) r = ri;
    }
    idx->scopes.swap(kept);
    return r;
}

// orr_index_delete_rows: the newly deleted positions (device, n of them) leave every scope of the shard.
static int scopes_drop_positions(orr_index *idx, const int64_t *d_pos, int64_t n)
{
    std::lock_guard<std::mutex> g(idx->scope_mu);
    return change_scopes(idx, [&](size_t, orr_scope *sc) -> int {
        Timed t(idx, "scope_clear_positions", 12.0 * (double)n);
        HIP_TRY(orr::launch_scope_clear_positions(sc->bm, sc->words, d_pos, n, idx->stream));
        return ORR_OK;
    });
}

// Carries every scope of a shard through a move of its rows (orr_index_compact, orr_index_insert_rows) in three steps: alloc
// (the new bitmaps, before the first row moves: ORR_ENOMEM leaves every scope as it was), run (ONE scope_remap launch for all
// scopes, while the source list is still there), commit (the scopes take their new arrays; the counts are refreshed; a scope whose refresh fails is orphaned).  The
// caller holds LanePool::Exclusive; the struct holds the shard's scope_mu from alloc on, so no scope comes or goes meanwhile.
struct ScopeRemap {
    orr_index *idx = nullptr;
    std::unique_lock<std::mutex> reg;
    int64_t new_rows = 0, new_words = 0;
    std::vector<uint32_t *> bm, chunks;                // the new arrays, one pair per scope of idx->scopes
    DevBuf ptrs;                                       // device: [old bitmaps x G][new bitmaps x G]
    bool committed = false;
    ~ScopeRemap()
    {
        if (!committed) for (size_t i = 0; i < bm.size(); ++i) free_scope_arrays(bm[i], chunks[i]);
        ptrs.release();
    }
    int alloc(orr_index *index, int64_t rows)
    {
        idx = index; new_rows = rows;
        reg = std::unique_lock<std::mutex>(idx->scope_mu);
        const size_t G = idx->scopes.size();
        if (G == 0) return ORR_OK;
        for (size_t i = 0; i < G; ++i) {
            uint32_t *b = nullptr, *c = nullptr;
            ORR_TRY(alloc_scope_arrays(rows, &b, &c, &new_words));
            bm.push_back(b); chunks.push_back(c);
        }
        return ptrs.reserve(sizeof(void *) * 2 * G);
    }
    // destination row d < first keeps its bit, row first + r takes that of old position src[r] (device), none when negative
    int run(const int64_t *src, int64_t first)
    {
        const size_t G = bm.size();
        if (G == 0) return ORR_OK;
        hipStream_t s = idx->stream;
        std::vector<const void *> h(2 * G);
        for (size_t i = 0; i < G; ++i) { h[i] = idx->scopes[i]->bm; h[G + i] = bm[i]; }
        HIP_TRY(hipMemcpy(ptrs.p, h.data(), sizeof(void *) * 2 * G, hipMemcpyHostToDevice));
        {
            Timed t(idx, "scope_remap", 8.0 * (double)(new_rows - first) + 8.0 * (double)G * (double)new_words);
            HIP_TRY(orr::launch_scope_remap(src, first, new_rows, new_words, ptrs.as<const uint32_t *>(), idx->scopes[0]->words,
                                            reinterpret_cast<uint32_t *const *>(ptrs.as<uint32_t *>() + G), (int32_t)G, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        collect_events(idx);
        return ORR_OK;
    }
    int commit()
    {
        committed = true;
        if (bm.empty()) return ORR_OK;
        return change_scopes(idx, [&](size_t i, orr_scope *sc) -> int {
            free_scope_arrays(sc->bm, sc->chunks);
            sc->bm = bm[i]; sc->chunks = chunks[i];
            sc->n_rows = new_rows; sc->words = new_words;
            return ORR_OK;
        });
    }
};

// Carries every registered orr_keys of a shard through the same move, in the same three steps: alloc (the new columns, in the
// allocation phase: ORR_ENOMEM leaves every column as it was), run (ONE keys_remap launch for all columns, from the sources
// scope_remap reads), commit (the handles take their new columns).  A new row reads ORR_KEY_NONE until the host sets it.  The
// caller holds LanePool::Exclusive and -- through its ScopeRemap, whose alloc comes first -- the shard's scope_mu.
struct KeysRemap {
    orr_index *idx = nullptr;
    int64_t new_rows = 0;
    std::vector<int64_t *> cols;                       // the new columns, one per handle of idx->key_cols
    DevBuf ptrs;                                       // device: [old columns x G][new columns x G]
    bool committed = false;
    ~KeysRemap()
    {
        if (!committed) for (int64_t *c : cols) if (c) (void)hipFree(c);
        ptrs.release();
    }
    int alloc(orr_index *index, int64_t rows)
    {
        idx = index; new_rows = rows;
        const size_t G = idx->key_cols.size();
        if (G == 0) return ORR_OK;
        for (size_t i = 0; i < G; ++i) {
            int64_t *c = nullptr;
            ORR_TRY(dev_alloc(&c, (size_t)std::max<int64_t>(rows, 1)));
            cols.push_back(c);
        }
        return ptrs.reserve(sizeof(void *) * 2 * G);
    }
    int run(const int64_t *src, int64_t first)
    {
        const size_t G = cols.size();
        if (G == 0) return ORR_OK;
        hipStream_t s = idx->stream;
        std::vector<const void *> h(2 * G);
        for (size_t i = 0; i < G; ++i) { h[i] = idx->key_cols[i]->d_key; h[G + i] = cols[i]; }
        HIP_TRY(hipMemcpy(ptrs.p, h.data(), sizeof(void *) * 2 * G, hipMemcpyHostToDevice));
        {
            Timed t(idx, "keys_remap", 8.0 * (double)(new_rows - first) + 16.0 * (double)G * (double)new_rows);
            HIP_TRY(orr::launch_keys_remap(src, first, new_rows, ptrs.as<const int64_t *>(), reinterpret_cast<int64_t *const *>(ptrs.as<int64_t *>() + G),
                                           (int32_t)G, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        collect_events(idx);
        return ORR_OK;
    }
    void commit()
    {
        committed = true;
        for (size_t i = 0; i < cols.size(); ++i) {
            orr_keys *k = idx->key_cols[i];
            std::unique_lock<std::shared_mutex> w(k->mu);
            if (k->d_key) (void)hipFree(k->d_key);
            k->d_key = cols[i];
            k->n_rows = new_rows;
        }
    }
};

int orr_index_delete_rows(orr_index *idx, int64_t n, const int64_t *row_ids, int64_t *out_deleted)
{
    if (out_deleted) *out_deleted = 0;
    if (!idx || n < 0 || (n > 0 && !row_ids)) return fail(ORR_EINVAL, "orr_index_delete_rows: bad argument");
    LanePool::Exclusive all(pool_of(idx));             // no search in flight on any lane while the rows change
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_delete_rows: the index is not sealed");
    if (idx->is_view) return fail(ORR_EINVAL, "orr_index_delete_rows: delete on the owning index, not on a view");
    if (n == 0 || idx->n_rows == 0) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    const size_t rows = (size_t)idx->n_rows;
    std::vector<int64_t> want((size_t)n);
    HIP_TRY(hipMemcpy(want.data(), row_ids, sizeof(int64_t) * (size_t)n, hipMemcpyDefault));
    std::vector<std::pair<int64_t, int64_t>> found;
    ORR_TRY(live_rows_of_ids(idx, want, found));
    std::vector<int64_t> fresh;
    for (const auto &f : found) fresh.push_back(f.first);
    std::sort(fresh.begin(), fresh.end());
    fresh.erase(std::unique(fresh.begin(), fresh.end()), fresh.end());
    if (fresh.empty()) return ORR_OK;
    if ((idx->dead.size() + fresh.size()) * 4 > rows)
        return fail(ORR_ESTATE, "orr_index_delete_rows: more than a quarter of the shard's %lld rows would be deleted: rebuild the shard",
                    (long long)idx->n_rows);
    std::vector<int64_t> merged(idx->dead.size() + fresh.size());
    std::merge(idx->dead.begin(), idx->dead.end(), fresh.begin(), fresh.end(), merged.begin());
    DevBuf tmp;
    ORR_TRY(tmp.reserve(sizeof(int64_t) * fresh.size()));
    int r = ORR_OK;
    if (hipMemcpy(tmp.p, fresh.data(), sizeof(int64_t) * fresh.size(), hipMemcpyHostToDevice) != hipSuccess ||
        orr::launch_tombstone_rows(tmp.as<int64_t>(), (int32_t)fresh.size(), idx->d_norm_b, idx->d_created, idx->stream) != hipSuccess ||
        hipStreamSynchronize(idx->stream) != hipSuccess)
        r = fail(ORR_EDEVICE, "orr_index_delete_rows: device update failed");
    if (r == ORR_OK) r = scopes_drop_positions(idx, tmp.as<int64_t>(), (int64_t)fresh.size());
    tmp.release();
    ORR_TRY(r);
    ORR_TRY(idx->d_dead.reserve(sizeof(int64_t) * merged.size()));
    HIP_TRY(hipMemcpy(idx->d_dead.p, merged.data(), sizeof(int64_t) * merged.size(), hipMemcpyHostToDevice));
    idx->dead.swap(merged);
    idx->lanes.update_shared([&](LanePool::Shared &sh) { sh.dead_count = (int64_t)idx->dead.size(); });
    if (out_deleted) *out_deleted = (int64_t)fresh.size();
    return ORR_OK;
}

int orr_index_update_rows(orr_index *idx, int64_t n, const int64_t *row_ids, int32_t dim, const float *emb, int64_t *out_updated)
{
    if (out_updated) *out_updated = 0;
    if (!idx || n < 0 || (n > 0 && !row_ids)) return fail(ORR_EINVAL, "orr_index_update_rows: bad argument");
    if (n > 0 && dim != 0 && !emb) return fail(ORR_EINVAL, "orr_index_update_rows: emb is NULL with dim %d", dim);
    if (dim == 0 && emb) return fail(ORR_EINVAL, "orr_index_update_rows: dim 0 (rows without an embedding) takes emb = NULL");
    LanePool::Exclusive all(pool_of(idx));             // no search in flight on any lane while the rows change
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_update_rows: the index is not sealed");
    if (idx->is_view) return fail(ORR_EINVAL, "orr_index_update_rows: update the owning index, not a view");
    if (idx->dim == 0) return fail(ORR_ESTATE, "orr_index_update_rows: the index was created with dim 0: it holds no embeddings");
    if (dim != 0 && dim != idx->dim)
        return fail(ORR_EDIM, "orr_index_update_rows: dim %d differs from the index dimension %d", dim, idx->dim);
    if (n == 0 || idx->n_rows == 0) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    std::vector<int64_t> want((size_t)n);
    HIP_TRY(hipMemcpy(want.data(), row_ids, sizeof(int64_t) * (size_t)n, hipMemcpyDefault));
    {
        std::vector<int64_t> sorted(want);
        std::sort(sorted.begin(), sorted.end());
        const auto rep = std::adjacent_find(sorted.begin(), sorted.end());
        if (rep != sorted.end()) return fail(ORR_EINVAL, "orr_index_update_rows: row id %lld is listed twice", (long long)*rep);
    }
    std::vector<std::pair<int64_t, int64_t>> found;    // (position, input row), ascending input row
    ORR_TRY(live_rows_of_ids(idx, want, found));
    if (found.empty()) return ORR_OK;
    const int32_t D = idx->dim;
    const int64_t n_t = (int64_t)found.size();
    std::vector<int64_t> pos((size_t)n_t), src((size_t)n_t);
    for (int64_t t = 0; t < n_t; ++t) { pos[(size_t)t] = found[(size_t)t].first; src[(size_t)t] = found[(size_t)t].second; }
    // the input rows go through a bounded staging buffer (at most 256 MiB of rows per round, as compaction's bounce buffer):
    // exact norms of the staged rows by the kernel the seal uses, then one wave per target writes the row, its norm and the
    // shadows' rows in place
    const int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)sizeof(float) * D));
    const int64_t m_max = std::min<int64_t>(chunk, n);
    hipStream_t s = idx->stream;
    void *i8 = idx->i8_ready ? idx->emb_i8.p : nullptr;
    void *bf = idx->shadow_ready ? idx->emb_shadow.p : nullptr;
    DevBuf stage, norms, d_pos, d_src;
    auto body = [&]() -> int {
        ORR_TRY(stage.reserve(sizeof(float) * (size_t)m_max * D));
        ORR_TRY(norms.reserve(sizeof(double) * (size_t)m_max));
        ORR_TRY(d_pos.reserve(sizeof(int64_t) * (size_t)n_t));
        ORR_TRY(d_src.reserve(sizeof(int64_t) * (size_t)n_t));
        HIP_TRY(hipMemcpyAsync(d_pos.p, pos.data(), sizeof(int64_t) * (size_t)n_t, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_src.p, src.data(), sizeof(int64_t) * (size_t)n_t, hipMemcpyHostToDevice, s));
        if (dim == 0) HIP_TRY(hipMemsetAsync(stage.p, 0, sizeof(float) * (size_t)m_max * D, s));      // zero rows, norm 0 (as append)
        int64_t t0 = 0;
        for (int64_t j0 = 0; j0 < n && t0 < n_t; j0 += chunk) {
            const int64_t m = std::min<int64_t>(chunk, n - j0);
            int64_t t1 = t0;
            while (t1 < n_t && src[(size_t)t1] < j0 + m) ++t1;
            if (t1 == t0) continue;                                   // no live row among these ids
            if (dim != 0)
                HIP_TRY(hipMemcpyAsync(stage.p, emb + (size_t)j0 * D, sizeof(float) * (size_t)m * D, hipMemcpyDefault, s));
            HIP_TRY(orr::launch_dot_exact(stage.as<float>(), m, D, nullptr, 1, true, norms.as<double>(), m, s));
            HIP_TRY(orr::launch_update_rows(stage.as<float>(), norms.as<double>(), d_pos.as<int64_t>() + t0, d_src.as<int64_t>() + t0, j0,
                                            t1 - t0, D, idx->d_emb, idx->d_norm_b, i8, idx->i8_scale.as<float>(), idx->i8_rel_err.as<float>(),
                                            idx->i8_rel_hat.as<float>(), idx->i8_rowf.as<float4>(), bf, s));
            t0 = t1;
        }
        HIP_TRY(hipStreamSynchronize(s));
        return ORR_OK;
    };
    const int r = body();
    stage.release(); norms.release(); d_pos.release(); d_src.release();
    if (r != ORR_OK) return r == ORR_ENOMEM ? r : fail(ORR_EDEVICE, "orr_index_update_rows: device update failed: %s", orr_last_error());
    if (out_updated) *out_updated = n_t;
    return ORR_OK;
}

int orr_index_compact(orr_index *idx, int64_t *out_removed)
{
    if (out_removed) *out_removed = 0;
    if (!idx) return fail(ORR_EINVAL, "orr_index_compact: null index");
    if (idx->is_view) return fail(ORR_EINVAL, "orr_index_compact: compact the owning index, not a view");
    LanePool::Exclusive all(pool_of(idx));             // no search in flight while rows move
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_compact: the index is not sealed");
    if (idx->user_views.load() > 0)
        return fail(ORR_ESTATE, "orr_index_compact: %d view(s) of this index are alive (orr_index_view): destroy them first", idx->user_views.load());
    if (idx->dead.empty()) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    const int64_t n = idx->n_rows, n_dead = (int64_t)idx->dead.size(), n_new = n - n_dead;
    // live positions, ascending (= the new candidate order), and how far each old position moves up
    std::vector<int64_t> live((size_t)n_new);
    std::vector<uint32_t> shift((size_t)n + 1);
    {
        size_t d = 0, w = 0;
        for (int64_t p = 0; p < n; ++p) {
            shift[(size_t)p] = (uint32_t)d;
            if (d < idx->dead.size() && idx->dead[d] == p) { ++d; continue; }
            live[w++] = p;
        }
        shift[(size_t)n] = (uint32_t)d;
    }
    ScopeRemap scopes;                                 // (deleted rows are already absent from every scope: the remap only closes gaps)
    ORR_TRY(scopes.alloc(idx, n_new));
    KeysRemap key_cols;                                // (under the scope_mu `scopes` holds)
    ORR_TRY(key_cols.alloc(idx, n_new));
    DevBuf d_live;
    ORR_TRY(d_live.reserve(sizeof(int64_t) * (size_t)std::max<int64_t>(n_new, 1)));
    int r = ORR_OK;
    auto body = [&]() -> int {
        if (n_new > 0) HIP_TRY(hipMemcpy(d_live.p, live.data(), sizeof(int64_t) * (size_t)n_new, hipMemcpyHostToDevice));
        // ---- embeddings: IN PLACE, chunk by chunk through a bounce buffer (a second copy of a 150 GB shard does not fit).  Rows only
        // move towards lower positions, and chunks go in ascending order, so a chunk's destination never reaches rows a later chunk
        // still has to read.
        if (idx->dim > 0 && n_new > 0) {
            const int64_t first_moved = idx->dead.front();                  // rows in front of the first deleted one stay where they are
            const int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)sizeof(float) * idx->dim));
            DevBuf bounce;
            ORR_TRY(bounce.reserve(sizeof(float) * (size_t)chunk * idx->dim));
            int64_t w0 = first_moved;                                       // live[w0] is the first row that moves (w0 rows in front of it are live)
            w0 = (int64_t)(std::lower_bound(live.begin(), live.end(), first_moved) - live.begin());
            for (int64_t w = w0; w < n_new; w += chunk) {
                const int64_t m = std::min<int64_t>(chunk, n_new - w);
                const hipError_t e1 = orr::launch_gather_rows_f32(idx->d_emb, bounce.as<float>(), d_live.as<int64_t>() + w, m, idx->dim, s);
                if (e1 != hipSuccess) { bounce.release(); return fail(ORR_EDEVICE, "orr_index_compact: gather failed: %s", hipGetErrorString(e1)); }
                const hipError_t e2 = hipMemcpyAsync(idx->d_emb + (size_t)w * idx->dim, bounce.p, sizeof(float) * (size_t)m * idx->dim, hipMemcpyDeviceToDevice, s);
                if (e2 != hipSuccess) { bounce.release(); return fail(ORR_EDEVICE, "orr_index_compact: copy failed: %s", hipGetErrorString(e2)); }
            }
            const hipError_t e3 = hipStreamSynchronize(s);
            bounce.release();
            if (e3 != hipSuccess) return fail(ORR_EDEVICE, "orr_index_compact: %s", hipGetErrorString(e3));
        }
        // ---- per-row scalars: gathered into new arrays (8 bytes per row each)
        int64_t *nc = nullptr, *nr = nullptr, *nn = nullptr;
        ORR_TRY(dev_alloc(&nc, (size_t)idx->cap_rows));
        ORR_TRY(dev_alloc(&nr, (size_t)idx->cap_rows));
        ORR_TRY(dev_alloc(&nn, (size_t)std::max<int64_t>(n, 1)));
        if (n_new > 0) {
            HIP_TRY(orr::launch_gather_i64(idx->d_created, nc, d_live.as<int64_t>(), n_new, s));
            HIP_TRY(orr::launch_gather_i64(idx->d_row_ids, nr, d_live.as<int64_t>(), n_new, s));
            HIP_TRY(orr::launch_gather_i64(reinterpret_cast<const int64_t *>(idx->d_norm_b), nn, d_live.as<int64_t>(), n_new, s));   // (the norms as bit patterns)
        }
        HIP_TRY(hipStreamSynchronize(s));
        (void)hipFree(idx->d_created); idx->d_created = nc;
        (void)hipFree(idx->d_row_ids); idx->d_row_ids = nr;
        (void)hipFree(idx->d_norm_b); idx->d_norm_b = reinterpret_cast<double *>(nn);
        // ---- token index: every posting list loses the deleted positions and is renumbered (on the host: one pass over the postings)
        if (idx->n_postings > 0) {
            const size_t V = (size_t)idx->n_tokens;
            std::vector<uint64_t> off(V + 1), noff(V + 1);
            std::vector<uint32_t> rows((size_t)idx->n_postings);
            HIP_TRY(hipMemcpy(off.data(), idx->d_post_off, sizeof(uint64_t) * (V + 1), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(rows.data(), idx->d_post_rows, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost));
            size_t w = 0;
            for (size_t t = 0; t < V; ++t) {
                noff[t] = w;
                for (uint64_t i = off[t]; i < off[t + 1]; ++i) {
                    const uint32_t p = rows[(size_t)i];
                    if (shift[(size_t)p + 1] != shift[(size_t)p]) continue;       // a deleted row
                    rows[w++] = p - shift[(size_t)p];
                }
            }
            noff[V] = w;
            HIP_TRY(hipMemcpy(idx->d_post_off, noff.data(), sizeof(uint64_t) * (V + 1), hipMemcpyHostToDevice));
            if (w) HIP_TRY(hipMemcpy(idx->d_post_rows, rows.data(), sizeof(uint32_t) * w, hipMemcpyHostToDevice));
            idx->n_postings = w;
        }
        ORR_TRY(key_cols.run(d_live.as<int64_t>(), 0));
        return scopes.run(d_live.as<int64_t>(), 0);    // (while d_live is there)
    };
    r = body();
    d_live.release();
    if (r != ORR_OK) return r;                         // (a failure half way leaves the shard unusable: the caller rebuilds it)
    // ---- host mirrors
    {
        std::vector<int64_t> hc((size_t)n_new);
        std::vector<uint32_t> hl((size_t)n_new);
        for (int64_t w = 0; w < n_new; ++w) { hc[(size_t)w] = idx->h_created[(size_t)live[(size_t)w]]; hl[(size_t)w] = idx->h_clen[(size_t)live[(size_t)w]]; }
        idx->h_created.swap(hc);
        idx->h_clen.swap(hl);
        idx->h_cprefix.assign((size_t)n_new + 1, 0);
        for (int64_t w = 0; w < n_new; ++w) idx->h_cprefix[(size_t)w + 1] = idx->h_cprefix[(size_t)w] + idx->h_clen[(size_t)w];
    }
    idx->n_rows = n_new;
    idx->dead.clear();
    idx->d_dead.release();
    idx->id_index.clear();
    drop_scope_table(idx, scopes.reg);
    // derived copies are rebuilt at the next search that wants them; the lanes' borrowed pointers die with the lanes
    idx->emb_shadow.release(); idx->shadow_ready = false; idx->shadow_failed = false;
    idx->emb_i8.release(); idx->i8_scale.release(); idx->i8_rel_err.release(); idx->i8_rel_hat.release(); idx->i8_rowf.release();
    idx->i8_ready = false; idx->i8_failed = false;
    idx->kw_clean.withdraw_bitmaps();
    idx->tok_bm.release(); idx->tok_bm_index.release(); idx->n_tok_bm = -1; idx->tok_bm_words = 0;
    idx->lanes.update_shared([](LanePool::Shared &sh) { sh.dead_count = 0; });
    for (orr_index *l : idx->lanes.drain()) orr_index_destroy(l);
    if (out_removed) *out_removed = n_dead;
    key_cols.commit();
    return scopes.commit();
}

namespace {

// wall-clock phases of orr_index_insert_rows among the kernel statistics (orr_index_set_profiling(1)): they are host-timed,
// each ends in a stream synchronise
void add_phase_stat(orr_index *idx, const char *name, std::chrono::steady_clock::time_point t0, double bytes)
{
    if (idx->profiling != 1) return;
    KernelStat &st = idx->stats[(size_t)stat_slot(idx, name)];
    st.launches += 1;
    st.total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    st.algo_bytes += bytes;
}

// room for `rows` rows of embeddings in a SEALED shard: 1.5 x like append, exactly `rows` when that does not fit.  The old
// array is freed only after the copy, so this needs a second copy of the embeddings for a moment.  Only d_emb grows: after
// the seal the per-row scalar arrays are never written behind n_rows, they are replaced whole (compaction, insertion) by
// arrays of cap_rows entries.
int grow_sealed_capacity(orr_index *idx, int64_t rows)
{
    if (rows <= idx->cap_rows) return ORR_OK;
    int64_t nc = std::max<int64_t>(std::max<int64_t>(rows, idx->cap_rows + idx->cap_rows / 2), 1024);
    if (idx->dim > 0) {
        int r = dev_grow(&idx->d_emb, (size_t)idx->n_rows * idx->dim, (size_t)nc * idx->dim, idx->stream);
        if (r == ORR_ENOMEM && nc > rows) {
            (void)hipGetLastError();
            nc = rows;
            r = dev_grow(&idx->d_emb, (size_t)idx->n_rows * idx->dim, (size_t)nc * idx->dim, idx->stream);
        }
        ORR_TRY(r);
    }
    idx->cap_rows = nc;
    return ORR_OK;
}

}  // namespace

int orr_index_insert_rows(orr_index *idx, int64_t n, int32_t dim, const float *emb, const int64_t *created_ticks,
                          const uint8_t *content_lower, const uint64_t *content_off, const int64_t *row_ids, int64_t *out_inserted)
{
    if (out_inserted) *out_inserted = 0;
    if (!idx) return fail(ORR_EINVAL, "orr_index_insert_rows: null index");
    if (n < 0) return fail(ORR_EINVAL, "orr_index_insert_rows: negative row count");
    if (n > 0 && !row_ids)
        return fail(ORR_EINVAL, "orr_index_insert_rows: row_ids are required (positions are not unique ids once a shard was compacted)");
    if (n > 0 && (!created_ticks || !content_off)) return fail(ORR_EINVAL, "orr_index_insert_rows: created_ticks and content_off are required");
    if (n > 0 && dim != 0 && !emb) return fail(ORR_EINVAL, "orr_index_insert_rows: emb is NULL with dim %d", dim);
    if (dim == 0 && emb) return fail(ORR_EINVAL, "orr_index_insert_rows: dim 0 (rows without an embedding) takes emb = NULL");
    if (idx->is_view) return fail(ORR_EINVAL, "orr_index_insert_rows: insert into the owning index, not into a view");
    LanePool::Exclusive all(pool_of(idx));             // no search in flight while rows move
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_insert_rows: the index is not sealed (orr_index_append takes rows before the seal)");
    if (idx->user_views.load() > 0)
        return fail(ORR_ESTATE, "orr_index_insert_rows: %d view(s) of this index are alive (orr_index_view): destroy them first", idx->user_views.load());
    if (dim != 0 && dim != idx->dim)
        return fail(ORR_EDIM, "orr_index_insert_rows: dim %d differs from the index dimension %d", dim, idx->dim);
    if (idx->n_rows + n >= (int64_t)0xFFFFFFFFll) return fail(ORR_EINVAL, "orr_index_insert_rows: more than 2^32-1 rows in one shard");
    if (n == 0) return ORR_OK;
    ORR_TRY(bind_device(idx));
    hipStream_t s = idx->stream;
    const int32_t D = idx->dim;
    const int64_t n_old = idx->n_rows, total = n_old + n;
    auto t_phase = std::chrono::steady_clock::now();

    // ---- the new rows' scalars and text come to the host; the merge plan (orr_insert_plan.h)
    std::vector<int64_t> new_ticks((size_t)n), new_ids((size_t)n);
    std::vector<uint64_t> off((size_t)n + 1);
    HIP_TRY(hipMemcpy(new_ticks.data(), created_ticks, sizeof(int64_t) * (size_t)n, hipMemcpyDefault));
    HIP_TRY(hipMemcpy(new_ids.data(), row_ids, sizeof(int64_t) * (size_t)n, hipMemcpyDefault));
    HIP_TRY(hipMemcpy(off.data(), content_off, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDefault));
    std::vector<uint32_t> new_len((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (off[(size_t)i + 1] < off[(size_t)i]) return fail(ORR_EINVAL, "orr_index_insert_rows: content_off is not monotone at row %lld", (long long)i);
        if (off[(size_t)i + 1] - off[(size_t)i] >= (1ull << 31)) return fail(ORR_EINVAL, "orr_index_insert_rows: content of row %lld exceeds 2 GiB", (long long)i);
        new_len[(size_t)i] = (uint32_t)(off[(size_t)i + 1] - off[(size_t)i]);
    }
    const uint64_t text_bytes = off[(size_t)n] - off[0];
    if (text_bytes > 0 && !content_lower) return fail(ORR_EINVAL, "orr_index_insert_rows: content_lower is NULL");
    std::vector<uint8_t> text((size_t)text_bytes + 16, 0x20);
    if (text_bytes) HIP_TRY(hipMemcpy(text.data(), content_lower + off[0], (size_t)text_bytes, hipMemcpyDefault));
    const orr::InsertPlan pl = orr::make_insert_plan(idx->h_created.data(), n_old, new_ticks.data(), n);
    const int64_t first = pl.first_moved, n_moved = total - first;     // rows in front of `first` stay where they are

    // ---- token index: the new rows' own index (in merged rank order), merged on the host into the shard's (one pass over the
    // old postings, as compaction's renumbering; the old text left HBM at the seal and is not needed)
    std::vector<int64_t> r_ticks((size_t)n), r_ids((size_t)n);
    orr::TokenIndexHost ti_old, ti_new;
    {
        std::vector<uint64_t> r_start((size_t)n);
        std::vector<uint32_t> r_len((size_t)n);
        for (int64_t k = 0; k < n; ++k) {
            const size_t j = (size_t)pl.order[(size_t)k];
            r_ticks[(size_t)k] = new_ticks[j]; r_ids[(size_t)k] = new_ids[j];
            r_start[(size_t)k] = off[j] - off[0]; r_len[(size_t)k] = new_len[j];
        }
        orr::TokenIndexHost ti_add;
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        orr::build_token_index(text.data(), r_start.data(), r_len.data(), n, (int)std::min(hw, 32u), ti_add);
        const size_t V = (size_t)idx->n_tokens;
        ti_old.vstart.resize(V); ti_old.vlen.resize(V); ti_old.post_off.assign(V + 1, 0); ti_old.post_rows.resize((size_t)idx->n_postings);
        if (V) {
            HIP_TRY(hipMemcpy(ti_old.vstart.data(), idx->d_vstart, sizeof(uint64_t) * V, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(ti_old.vlen.data(), idx->d_vlen, sizeof(uint32_t) * V, hipMemcpyDeviceToHost));
            ti_old.vpool.resize((size_t)orr::vocab_pool_bytes(ti_old));
            HIP_TRY(hipMemcpy(ti_old.vpool.data(), idx->d_vpool, ti_old.vpool.size(), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(ti_old.post_off.data(), idx->d_post_off, sizeof(uint64_t) * (V + 1), hipMemcpyDeviceToHost));
        }
        if (idx->n_postings) HIP_TRY(hipMemcpy(ti_old.post_rows.data(), idx->d_post_rows, sizeof(uint32_t) * ti_old.post_rows.size(), hipMemcpyDeviceToHost));
        orr::merge_token_index(ti_old, ti_add, pl, ti_new);
        ti_old = orr::TokenIndexHost();
    }
    add_phase_stat(idx, "insert_token_index_host", t_phase, 4.0 * (double)ti_new.post_rows.size());
    std::vector<int64_t> src((size_t)n_moved);
    orr::plan_sources(pl, first, total, src.data());
    const std::vector<int64_t> new_dead = orr::remap_dead(pl, idx->dead);

    // ---- every allocation comes before the first row moves: ORR_ENOMEM leaves the shard as it was
    const int64_t chunk = D > 0 ? std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)sizeof(float) * D)) : total;
    const bool old_rows_move = first < n_old;
    ORR_TRY(grow_sealed_capacity(idx, total));
    struct Fresh {
        int64_t *created = nullptr, *ids = nullptr, *norms = nullptr, *src = nullptr, *add_ticks = nullptr, *add_ids = nullptr, *add_norms = nullptr;
        uint8_t *vpool = nullptr; uint64_t *vstart = nullptr, *post_off = nullptr; uint32_t *vlen = nullptr, *post_rows = nullptr;
        DevBuf stage, bounce;
        ~Fresh()
        {
            for (void *p : {(void *)created, (void *)ids, (void *)norms, (void *)src, (void *)add_ticks, (void *)add_ids, (void *)add_norms,
                            (void *)vpool, (void *)vstart, (void *)post_off, (void *)vlen, (void *)post_rows})
                if (p) (void)hipFree(p);
            stage.release(); bounce.release();
        }
    } fr;
    const size_t cap = (size_t)std::max<int64_t>(idx->cap_rows, 1);
    ORR_TRY(dev_alloc(&fr.created, cap));
    ORR_TRY(dev_alloc(&fr.ids, cap));
    ORR_TRY(dev_alloc(&fr.norms, cap));
    ORR_TRY(dev_alloc(&fr.src, (size_t)n_moved));
    ORR_TRY(dev_alloc(&fr.add_ticks, (size_t)n));
    ORR_TRY(dev_alloc(&fr.add_ids, (size_t)n));
    ORR_TRY(dev_alloc(&fr.add_norms, (size_t)n));
    ORR_TRY(dev_alloc(&fr.vpool, ti_new.vpool.size() + orr::kScanPoolSlack));
    ORR_TRY(dev_alloc(&fr.vstart, ti_new.vstart.size()));
    ORR_TRY(dev_alloc(&fr.vlen, ti_new.vlen.size()));
    ORR_TRY(dev_alloc(&fr.post_off, ti_new.post_off.size()));
    ORR_TRY(dev_alloc(&fr.post_rows, ti_new.post_rows.size()));
    if (D > 0) {
        ORR_TRY(fr.stage.reserve(sizeof(float) * (size_t)std::min<int64_t>(chunk, n) * D));
        if (old_rows_move) ORR_TRY(fr.bounce.reserve(sizeof(float) * (size_t)std::min<int64_t>(chunk, n_moved) * D));
    }
    if (!new_dead.empty()) ORR_TRY(idx->d_dead.reserve(sizeof(int64_t) * new_dead.size()));
    ScopeRemap scopes;                                 // the grown bitmaps of every scope handle
    ORR_TRY(scopes.alloc(idx, total));
    KeysRemap key_cols;                                // the grown columns of every orr_keys (under the scope_mu `scopes` holds)
    ORR_TRY(key_cols.alloc(idx, total));

    auto body = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(fr.src, src.data(), sizeof(int64_t) * (size_t)n_moved, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(fr.add_ticks, r_ticks.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(fr.add_ids, r_ids.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(fr.add_norms, 0, sizeof(double) * (size_t)n, s));
        // ---- embeddings: IN PLACE.  Rows only move towards higher positions, so the destination chunks go from the LAST to the
        // first: a chunk's destination never reaches rows an earlier chunk (in position) still has to read.  A chunk none of whose
        // old sources lies inside it is written directly; the others pass through the bounce buffer, as in compaction.  The new
        // rows of a chunk come through the staging buffer, where their exact norms are taken by the kernel the seal uses.
        t_phase = std::chrono::steady_clock::now();
        if (D > 0) {
            if (dim == 0) HIP_TRY(hipMemsetAsync(fr.stage.p, 0, sizeof(float) * (size_t)std::min<int64_t>(chunk, n) * D, s));   // zero rows, norm 0 (as append)
            for (int64_t d1 = total; d1 > first;) {
                const int64_t d0 = std::max<int64_t>(first, d1 - chunk), m = d1 - d0;
                const int64_t k0 = (int64_t)(std::lower_bound(pl.new_pos.begin(), pl.new_pos.end(), d0) - pl.new_pos.begin());
                const int64_t k1 = (int64_t)(std::lower_bound(pl.new_pos.begin(), pl.new_pos.end(), d1) - pl.new_pos.begin());
                if (k1 > k0 && dim != 0) {
                    for (int64_t k = k0; k < k1;) {                                 // runs of consecutive input rows go in one copy
                        int64_t e = k + 1;
                        while (e < k1 && pl.order[(size_t)e] == pl.order[(size_t)e - 1] + 1) ++e;
                        HIP_TRY(hipMemcpyAsync(fr.stage.as<float>() + (size_t)(k - k0) * D, emb + (size_t)pl.order[(size_t)k] * D,
                                               sizeof(float) * (size_t)(e - k) * D, hipMemcpyDefault, s));
                        k = e;
                    }
                    HIP_TRY(orr::launch_dot_exact(fr.stage.as<float>(), k1 - k0, D, nullptr, 1, true, reinterpret_cast<double *>(fr.add_norms) + k0, k1 - k0, s));
                }
                const int64_t p_hi = d1 - k1;                                       // old positions [d0 - k0, p_hi) land in this chunk
                const bool direct = p_hi <= d0 - k0 || p_hi <= d0;
                float *dst = idx->d_emb + (size_t)d0 * D;
                {
                    Timed t(idx, direct ? "merge_rows_f32_direct" : "merge_rows_f32_bounce", 8.0 * (double)m * D);
                    HIP_TRY(orr::launch_merge_rows_f32(idx->d_emb, fr.stage.as<float>(), fr.src + (d0 - first), k0, direct ? dst : fr.bounce.as<float>(), m, D, s));
                }
                if (!direct) HIP_TRY(hipMemcpyAsync(dst, fr.bounce.p, sizeof(float) * (size_t)m * D, hipMemcpyDeviceToDevice, s));
                d1 = d0;
            }
            HIP_TRY(hipStreamSynchronize(s));
            collect_events(idx);
            add_phase_stat(idx, "insert_move_rows", t_phase, 8.0 * (double)n_moved * D);
        }
        // ---- per-row scalars: merged into new arrays through the same source list (the norms as bit patterns; a deleted row's
        // overwritten norm and timestamp travel with it)
        t_phase = std::chrono::steady_clock::now();
        if (first > 0) {
            HIP_TRY(hipMemcpyAsync(fr.created, idx->d_created, sizeof(int64_t) * (size_t)first, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(fr.ids, idx->d_row_ids, sizeof(int64_t) * (size_t)first, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(fr.norms, idx->d_norm_b, sizeof(double) * (size_t)first, hipMemcpyDeviceToDevice, s));
        }
        HIP_TRY(orr::launch_merge_i64(idx->d_created, fr.add_ticks, fr.src, fr.created + first, n_moved, s));
        HIP_TRY(orr::launch_merge_i64(idx->d_row_ids, fr.add_ids, fr.src, fr.ids + first, n_moved, s));
        HIP_TRY(orr::launch_merge_i64(reinterpret_cast<const int64_t *>(idx->d_norm_b), fr.add_norms, fr.src, fr.norms + first, n_moved, s));
        // ---- token index
        HIP_TRY(hipMemsetAsync(fr.vpool, 0x20, ti_new.vpool.size() + orr::kScanPoolSlack, s));
        if (!ti_new.vpool.empty()) HIP_TRY(hipMemcpyAsync(fr.vpool, ti_new.vpool.data(), ti_new.vpool.size(), hipMemcpyHostToDevice, s));
        if (!ti_new.vstart.empty()) {
            HIP_TRY(hipMemcpyAsync(fr.vstart, ti_new.vstart.data(), sizeof(uint64_t) * ti_new.vstart.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(fr.vlen, ti_new.vlen.data(), sizeof(uint32_t) * ti_new.vlen.size(), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipMemcpyAsync(fr.post_off, ti_new.post_off.data(), sizeof(uint64_t) * ti_new.post_off.size(), hipMemcpyHostToDevice, s));
        if (!ti_new.post_rows.empty())
            HIP_TRY(hipMemcpyAsync(fr.post_rows, ti_new.post_rows.data(), sizeof(uint32_t) * ti_new.post_rows.size(), hipMemcpyHostToDevice, s));
        if (!new_dead.empty()) HIP_TRY(hipMemcpyAsync(idx->d_dead.p, new_dead.data(), sizeof(int64_t) * new_dead.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        add_phase_stat(idx, "insert_scalars_and_upload", t_phase, 48.0 * (double)n_moved + 4.0 * (double)ti_new.post_rows.size());
        ORR_TRY(key_cols.run(fr.src, first));          // a new row has no key
        return scopes.run(fr.src, first);              // a new row is in no scope; fr.src goes with fr
    };
    const int r = body();
    if (r != ORR_OK)                                   // (rows may have moved: the shard is unusable, the caller rebuilds it)
        return fail(ORR_EDEVICE, "orr_index_insert_rows: failed part way, rebuild the shard: %s", std::string(orr_last_error()).c_str());
    std::swap(idx->d_created, fr.created);
    std::swap(idx->d_row_ids, fr.ids);
    { int64_t *old_norms = reinterpret_cast<int64_t *>(idx->d_norm_b); idx->d_norm_b = reinterpret_cast<double *>(fr.norms); fr.norms = old_norms; }
    std::swap(idx->d_vpool, fr.vpool); std::swap(idx->d_vstart, fr.vstart); std::swap(idx->d_vlen, fr.vlen);
    std::swap(idx->d_post_off, fr.post_off); std::swap(idx->d_post_rows, fr.post_rows);          // (fr frees the old arrays)
    idx->n_tokens = (int64_t)ti_new.vstart.size();
    idx->n_postings = ti_new.post_rows.size();
    // ---- host mirrors and what hangs on positions
    {
        std::vector<int64_t> hc = orr::merge_rows(pl, idx->h_created.data(), new_ticks.data());
        std::vector<uint32_t> hl = orr::merge_rows(pl, idx->h_clen.data(), new_len.data());
        idx->h_created.swap(hc);
        idx->h_clen.swap(hl);
        idx->h_cprefix.assign((size_t)total + 1, 0);
        for (int64_t p = 0; p < total; ++p) idx->h_cprefix[(size_t)p + 1] = idx->h_cprefix[(size_t)p] + idx->h_clen[(size_t)p];
    }
    idx->n_rows = total;
    const int scopes_r = scopes.commit();              // (reported at the end: the rows are in whatever it says)
    key_cols.commit();
    idx->dead = new_dead;                              // (their number is unchanged: the lanes' shared dead_count stays)
    idx->id_index.clear();
    drop_scope_table(idx, scopes.reg);
    idx->n_vlong = -1; idx->n_vmid = 0;
    idx->kw_clean.withdraw_bitmaps();
    idx->tok_bm.release(); idx->tok_bm_index.release(); idx->n_tok_bm = -1; idx->tok_bm_words = 0;
    for (orr_index *l : idx->lanes.drain()) orr_index_destroy(l);      // they borrow arrays that were replaced; remade on demand
    // ---- a shadow that was ready is rebuilt now, from the moved rows, by the routine set_option("two_stage") uses: the next
    // search does not pay for it.  One that did not exist stays unbuilt.
    t_phase = std::chrono::steady_clock::now();
    const bool had_i8 = idx->i8_ready, had_bf16 = idx->shadow_ready;
    idx->i8_ready = false; idx->i8_failed = false; idx->shadow_ready = false; idx->shadow_failed = false;
    auto drop_i8 = [idx] { idx->emb_i8.release(); idx->i8_scale.release(); idx->i8_rel_err.release(); idx->i8_rel_hat.release(); idx->i8_rowf.release(); };
    // buffers too small for the grown shard go BEFORE the rebuild asks how much memory is free; buffers that still fit are used again
    if (!had_i8 || idx->emb_i8.cap < orr::i8_tiled_bytes(total, D) || idx->i8_rowf.cap < sizeof(float4) * (size_t)total) drop_i8();
    if (!had_bf16 || idx->emb_shadow.cap < orr::bf16_tiled_bytes(total, D)) idx->emb_shadow.release();
    if (out_inserted) *out_inserted = n;
    // The rows are in and the shard is whole whatever happens to a shadow: one that cannot be rebuilt now (no room, or a HIP error
    // in its build) is dropped, nothing stays marked as failed, and the next search that wants it tries again as on a new shard.
    if (had_i8 && (ensure_i8_shadow(idx) != ORR_OK || !idx->i8_ready)) { (void)hipGetLastError(); drop_i8(); idx->i8_ready = false; idx->i8_failed = false; }
    if (had_bf16 && (ensure_shadow(idx) != ORR_OK || !idx->shadow_ready)) { (void)hipGetLastError(); idx->emb_shadow.release(); idx->shadow_ready = false; idx->shadow_failed = false; }
    if (had_i8 || had_bf16) add_phase_stat(idx, "insert_shadow_rebuild", t_phase, 0.0);
    return scopes_r;
}

// the sticky options (orr_index_set_option) a lane has in common with its index (kw_hits_cap: a lane that had grown its own
// hit list starts from the index's size again and grows it again when a batch needs that)
static void copy_options(const orr_index *from, orr_index *to)
{
    to->opt_fuse_epilogue = from->opt_fuse_epilogue; to->opt_two_stage = from->opt_two_stage;
    to->opt_shard_pass = from->opt_shard_pass; to->opt_shard_topk = from->opt_shard_topk;
    to->kw_hits_cap = from->kw_hits_cap; to->dead_before = from->dead_before;
    to->opt_mask_screen = from->opt_mask_screen; to->opt_mask_part_rows = from->opt_mask_part_rows;
    to->near_band_cap = from->near_band_cap;
    to->opt_range_form = from->opt_range_form; to->opt_range_gemm = from->opt_range_gemm; to->opt_range_pair_cap = from->opt_range_pair_cap;
    to->range_buffer = from->range_buffer; to->range_list_cap = from->range_list_cap;
    to->opt_key_groups_slice = from->opt_key_groups_slice;
}

// a lane borrows whatever shadows its index has now
static void borrow_shadows(const orr_index *from, orr_index *to)
{
    to->emb_shadow.p = from->emb_shadow.p; to->shadow_ready = from->shadow_ready; to->shadow_failed = !from->shadow_ready;
    to->emb_i8.p = from->emb_i8.p; to->i8_scale.p = from->i8_scale.p; to->i8_rel_err.p = from->i8_rel_err.p;
    to->i8_rel_hat.p = from->i8_rel_hat.p; to->i8_rowf.p = from->i8_rowf.p;
    to->i8_ready = from->i8_ready; to->i8_failed = !from->i8_ready;
}

int orr_index_set_option(orr_index *idx, const char *name, int64_t value)
{
    if (!idx || !name) return fail(ORR_EINVAL, "orr_index_set_option: null argument");
    LanePool::Exclusive all(pool_of(idx));             // options apply to every lane of the index
    std::lock_guard<std::mutex> lock(idx->mu);
    if (strcmp(name, "max_lanes") == 0) {
        if (value < 1 || value > 16) return fail(ORR_EINVAL, "orr_index_set_option: max_lanes must be in 1 .. 16");
        if (idx->is_view) return fail(ORR_EINVAL, "orr_index_set_option: max_lanes applies to the owning index");
        idx->lanes.set_max_lanes((int)value);
        return ORR_OK;
    }
    if (strcmp(name, "fuse_epilogue") == 0) {
        idx->opt_fuse_epilogue = value != 0;
    } else if (strcmp(name, "dead_rows_before") == 0) {
        if (value < 0) return fail(ORR_EINVAL, "orr_index_set_option: dead_rows_before must be >= 0");
        idx->dead_before = value;
        idx->lanes.update_shared([value](LanePool::Shared &sh) { sh.dead_before = value; });
    } else if (strcmp(name, "kw_hits_cap") == 0) {
        if (value < 1 || value > (int64_t)0x7FFFFFFF) return fail(ORR_EINVAL, "orr_index_set_option: kw_hits_cap must be in 1 .. 2^31-1");
        idx->kw_hits_cap = (uint32_t)value;
    } else if (strcmp(name, "shard_topk") == 0) {
        if (value < 0 || value > 1 << 30) return fail(ORR_EINVAL, "orr_index_set_option: shard_topk must be >= 0");
        idx->opt_shard_topk = (int)value;
    } else if (strcmp(name, "shard_pass") == 0) {
        if (value < 0 || value > 2) return fail(ORR_EINVAL, "orr_index_set_option: shard_pass takes 0, 1 or 2");
        idx->opt_shard_pass = (int)value;
    } else if (strcmp(name, "mask_screen") == 0) {
        if (value < 0 || value > 2) return fail(ORR_EINVAL, "orr_index_set_option: mask_screen takes 0, 1 or 2");
        idx->opt_mask_screen = (int)value;
    } else if (strcmp(name, "mask_part_rows") == 0) {
        if (!mask::part_rows_valid(value))
            return fail(ORR_EINVAL, "orr_index_set_option: mask_part_rows must be in 1 .. %u", scope::kMaxScopeRows);
        idx->opt_mask_part_rows = value;
    } else if (strcmp(name, "near_band_cap") == 0) {
        if (!scope_near::band_cap_valid(value)) return fail(ORR_EINVAL, "orr_index_set_option: near_band_cap must be in 1 .. 2^31");
        idx->near_band_cap = value;
    } else if (strcmp(name, "range_pair_cap") == 0) {
        if (!range::pair_cap_valid(value)) return fail(ORR_EINVAL, "orr_index_set_option: range_pair_cap must be in 1 .. 2^31");
        idx->opt_range_pair_cap = value;
    } else if (strcmp(name, "range_buffer") == 0) {
        if (!range::buffer_valid(value)) return fail(ORR_EINVAL, "orr_index_set_option: range_buffer must be in 1 .. %lld", (long long)range::kMaxBuffer);
        idx->range_buffer = value;
        idx->range_list_cap = 0;
    } else if (strcmp(name, "key_groups_slice") == 0) {
        if (!key_groups::slice_option_valid(value)) return fail(ORR_EINVAL, "orr_index_set_option: key_groups_slice must be in 0 .. %d", key_groups::kMaxKeys);
        idx->opt_key_groups_slice = value;
    } else if (strcmp(name, "range_gemm") == 0) {
        if (!range_bulk::gemm_valid(value)) return fail(ORR_EINVAL, "orr_index_set_option: range_gemm takes 0, 1 or 2");
        idx->opt_range_gemm = (int)value;
    } else if (strcmp(name, "range_form") == 0) {
        if (!range::form_valid(value)) return fail(ORR_EINVAL, "orr_index_set_option: range_form takes 0, 1 or 2");
        idx->opt_range_form = (int)value;
    } else if (strcmp(name, "two_stage") == 0) {
        if (value < 0 || value > 2) return fail(ORR_EINVAL, "orr_index_set_option: two_stage takes 0, 1 or 2");
        idx->opt_two_stage = (int)value;
        if (value == 1) {
            HIP_TRY(hipSetDevice(idx->device));
            ORR_TRY(ensure_i8_shadow(idx));
            if (!idx->i8_ready) ORR_TRY(ensure_shadow(idx));
        }
        for_each_lane(idx, [&](orr_index *x) { if (x != idx) borrow_shadows(idx, x); });
    } else {
        return fail(ORR_EINVAL, "orr_index_set_option: unknown option %s", name);
    }
    for_each_lane(idx, [&](orr_index *x) { if (x != idx) copy_options(idx, x); });
    return ORR_OK;
}

static int make_view(orr_index *parent, orr_index **out, bool internal);

int orr_index_view(orr_index *parent, orr_index **out) { return make_view(parent, out, false); }

static int make_view(orr_index *parent, orr_index **out, bool internal)
{
    if (!parent || !out) return fail(ORR_EINVAL, "orr_index_view: null argument");
    *out = nullptr;
    std::lock_guard<std::mutex> lock(parent->mu);
    if (!parent->sealed) return fail(ORR_ESTATE, "orr_index_view: the index is not sealed");
    if (parent->is_view) return fail(ORR_EINVAL, "orr_index_view: take views of the owning index");
    HIP_TRY(hipSetDevice(parent->device));
    // the shadow is shared, so it has to exist before the view does -- but only shards the two-stage pass applies to get one
    if (parent->opt_two_stage == 1 && parent->n_rows >= 48 * (int64_t)orr::kSelSegRows) {
        ORR_TRY(ensure_i8_shadow(parent));
        if (!parent->i8_ready) ORR_TRY(ensure_shadow(parent));
    }
    ORR_TRY(ensure_vlong(parent));             // (before the view exists: a failure here must not leak it)
    ORR_TRY(ensure_token_bitmaps(parent));
    orr_index *v = new (std::nothrow) orr_index();
    if (!v) return fail(ORR_ENOMEM, "out of host memory");
    v->is_view = true;
    v->n_vlong = parent->n_vlong;
    v->n_vmid = parent->n_vmid;
    v->n_tok_bm = parent->n_tok_bm; v->tok_bm_words = parent->tok_bm_words;
    v->tok_bm.p = parent->tok_bm.p; v->tok_bm_index.p = parent->tok_bm_index.p;                                        // borrowed
    v->vlong_start.p = parent->vlong_start.p; v->vlong_len.p = parent->vlong_len.p; v->vlong_id.p = parent->vlong_id.p;   // borrowed
    v->parent = parent;
    v->device = parent->device; v->dim = parent->dim; v->row_base = parent->row_base;
    v->n_rows = parent->n_rows; v->cap_rows = parent->cap_rows;
    v->d_emb = parent->d_emb; v->d_created = parent->d_created; v->d_row_ids = parent->d_row_ids; v->d_norm_b = parent->d_norm_b;
    v->n_tokens = parent->n_tokens; v->d_vpool = parent->d_vpool; v->d_vstart = parent->d_vstart; v->d_vlen = parent->d_vlen;
    v->d_post_off = parent->d_post_off; v->d_post_rows = parent->d_post_rows; v->n_postings = parent->n_postings;
    v->sealed = true;
    copy_options(parent, v);
    borrow_shadows(parent, v);                         // (capacities stay 0: borrowed, never freed here)
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&v->stream_kw, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&v->stream_aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&v->ev_bm_clean, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&v->ev_inputs, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&v->ev_kw_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&v->ev_main_ready, hipEventDisableTiming) != hipSuccess ||
        !create_range_events(v->ev_range) ||
        hipEventCreateWithFlags(&v->ev_q, hipEventDisableTiming) != hipSuccess) {
        v->internal_lane = true;                       // (not counted yet: the destroy must not count it down)
        orr_index_destroy(v);
        return fail(ORR_EDEVICE, "cannot create streams on device %d", parent->device);
    }
    v->internal_lane = internal;
    if (!internal) parent->user_views.fetch_add(1);
    *out = v;
    return ORR_OK;
}

int orr_index_screen_dots(orr_index *idx, int32_t B, int32_t dim, const float *q, float *out)
{
    if (!idx || !q || !out || B <= 0) return fail(ORR_EINVAL, "orr_index_screen_dots: bad argument");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_screen_dots: the index is not sealed");
    if (dim != idx->dim || dim <= 0 || dim % 64 != 0) return fail(ORR_EINVAL, "orr_index_screen_dots: dim must equal the index dimension and be a multiple of 64");
    if (idx->n_rows <= 0) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    ORR_TRY(ensure_shadow(idx));
    if (!idx->shadow_ready) return fail(ORR_ENOMEM, "orr_index_screen_dots: the bf16 shadow does not fit in device memory");
    hipStream_t s = idx->stream;
    ORR_TRY(idx->ws_q.reserve(sizeof(float) * (size_t)B * dim));
    ORR_TRY(idx->ws_qtiled.reserve(orr::bf16_tiled_bytes(B, dim)));
    ORR_TRY(idx->ws_dotf.reserve(sizeof(float) * (size_t)B * (size_t)idx->n_rows));
    HIP_TRY(hipMemcpyAsync(idx->ws_q.p, q, sizeof(float) * (size_t)B * dim, hipMemcpyDefault, s));
    HIP_TRY(orr::launch_bf16_tiled(idx->ws_q.as<float>(), B, dim, idx->ws_qtiled.p, s));
    {
        Timed t(idx, "screen_bf16", 2.0 * (double)idx->n_rows * dim + 2.0 * (double)B * dim + 4.0 * (double)B * (double)idx->n_rows);
        HIP_TRY(orr::launch_screen_bf16(idx->ws_qtiled.p, B, idx->emb_shadow.p, 0, idx->n_rows, dim, idx->ws_dotf.as<float>(), idx->n_rows,
                                        nullptr, s));
    }
    HIP_TRY(hipMemcpyAsync(out, idx->ws_dotf.p, sizeof(float) * (size_t)B * (size_t)idx->n_rows, hipMemcpyDefault, s));
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(idx);
    return ORR_OK;
}

int orr_index_screen_i8_dots(orr_index *idx, int32_t B, int32_t dim, const float *q, int32_t form, int32_t nt_rows, int32_t *out_dots,
                             int8_t *out_iq, int8_t *out_ie)
{
    if (!idx || !q || B <= 0 || form < 0 || form > 2) return fail(ORR_EINVAL, "orr_index_screen_i8_dots: bad argument");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_screen_i8_dots: the index is not sealed");
    if (dim != idx->dim || dim <= 0 || dim % 128 != 0) return fail(ORR_EINVAL, "orr_index_screen_i8_dots: dim must equal the index dimension and be a multiple of 128");
    if (form > 0 && dim / 64 <= 6) return fail(ORR_EINVAL, "orr_index_screen_i8_dots: the four-wave forms need dim >= 448");
    if (idx->n_rows <= 0) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    ORR_TRY(ensure_i8_shadow(idx));
    if (!idx->i8_ready) return fail(ORR_ENOMEM, "orr_index_screen_i8_dots: the int8 shadow does not fit in device memory");
    hipStream_t s = idx->stream;
    const size_t n = (size_t)idx->n_rows;
    ORR_TRY(idx->ws_q.reserve(sizeof(float) * (size_t)B * dim));
    ORR_TRY(idx->ws_q8.reserve(2 * (size_t)B * dim));
    ORR_TRY(idx->ws_q8s1.reserve(sizeof(float) * (size_t)B));
    ORR_TRY(idx->ws_q8err.reserve(2 * sizeof(double) * (size_t)B));
    ORR_TRY(idx->ws_qtiled.reserve(orr::i8_tiled_bytes(B, dim)));
    HIP_TRY(hipMemcpyAsync(idx->ws_q.p, q, sizeof(float) * (size_t)B * dim, hipMemcpyDefault, s));
    // the same quantisation and tiling the searches use (one int8 level per query)
    HIP_TRY(orr::launch_i8_queries(idx->ws_q.as<float>(), B, dim, idx->ws_q8.p, idx->ws_q8s1.as<float>(), idx->ws_q8err.as<double>(), s,
                                   idx->ws_q8err.as<double>() + B));
    HIP_TRY(orr::launch_i8_tile_queries(idx->ws_q8.p, B, dim, idx->ws_qtiled.p, s));
    if (out_dots) {
        ORR_TRY(idx->ws_dotf.reserve(sizeof(int32_t) * (size_t)B * n));
        HIP_TRY(hipMemsetAsync(idx->ws_dotf.p, 0xAB, sizeof(int32_t) * (size_t)B * n, s));     // (an element the kernel never writes shows up as 0xABABABAB)
        ORR_TRY(idx->ws_tickets.reserve(sizeof(uint32_t) * 8 * 16));
        HIP_TRY(hipMemsetAsync(idx->ws_tickets.p, 0, sizeof(uint32_t) * 8 * 16, s));
        {
            Timed t(idx, form == 0 ? "screen_i8_dots_w8" : form == 1 ? "screen_i8_dots_w4" : "screen_i8_dots_w16",
                    1.0 * (double)n * dim + 1.0 * (double)B * dim + 4.0 * (double)B * (double)n);
            HIP_TRY(orr::launch_screen_i8_dots_raw(idx->ws_qtiled.p, B, idx->emb_i8.p, idx->n_rows, dim, idx->ws_dotf.as<int32_t>(),
                                                   idx->n_rows, form, nt_rows != 0, s, idx->ws_tickets.as<uint32_t>()));
        }
        HIP_TRY(hipMemcpyAsync(out_dots, idx->ws_dotf.p, sizeof(int32_t) * (size_t)B * n, hipMemcpyDefault, s));
    }
    if (out_iq) HIP_TRY(hipMemcpyAsync(out_iq, idx->ws_q8.p, (size_t)B * dim, hipMemcpyDefault, s));
    if (out_ie) {
        ORR_TRY(idx->ws_raw.reserve(n * (size_t)dim));
        HIP_TRY(orr::launch_i8_untile(idx->emb_i8.p, idx->n_rows, dim, idx->ws_raw.p, s));
        HIP_TRY(hipMemcpyAsync(out_ie, idx->ws_raw.p, n * (size_t)dim, hipMemcpyDefault, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(idx);
    return ORR_OK;
}

int orr_index_screen_i8_consts(orr_index *idx, int32_t B, int32_t dim, const float *q, float *out_scale, float *out_rel_err,
                               float *out_rel_hat, float *out_rowf, float *out_s1, double *out_err2, double *out_err2_level1,
                               int8_t *out_iq2)
{
    if (!idx || B < 0 || (B > 0 && !q)) return fail(ORR_EINVAL, "orr_index_screen_i8_consts: bad argument");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_screen_i8_consts: the index is not sealed");
    if (dim != idx->dim || dim <= 0 || dim % 128 != 0) return fail(ORR_EINVAL, "orr_index_screen_i8_consts: dim must equal the index dimension and be a multiple of 128");
    if (idx->n_rows <= 0) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    ORR_TRY(ensure_i8_shadow(idx));
    if (!idx->i8_ready) return fail(ORR_ENOMEM, "orr_index_screen_i8_consts: the int8 shadow does not fit in device memory");
    hipStream_t s = idx->stream;
    const size_t n = (size_t)idx->n_rows;
    if (out_scale) HIP_TRY(hipMemcpyAsync(out_scale, idx->i8_scale.p, sizeof(float) * n, hipMemcpyDefault, s));
    if (out_rel_err) HIP_TRY(hipMemcpyAsync(out_rel_err, idx->i8_rel_err.p, sizeof(float) * n, hipMemcpyDefault, s));
    if (out_rel_hat) HIP_TRY(hipMemcpyAsync(out_rel_hat, idx->i8_rel_hat.p, sizeof(float) * n, hipMemcpyDefault, s));
    if (out_rowf) HIP_TRY(hipMemcpyAsync(out_rowf, idx->i8_rowf.p, sizeof(float4) * n, hipMemcpyDefault, s));
    if (B > 0) {
        ORR_TRY(idx->ws_q.reserve(sizeof(float) * (size_t)B * dim));
        ORR_TRY(idx->ws_q8.reserve(2 * (size_t)B * dim));
        ORR_TRY(idx->ws_q8s1.reserve(sizeof(float) * (size_t)B));
        ORR_TRY(idx->ws_q8err.reserve(2 * sizeof(double) * (size_t)B));
        HIP_TRY(hipMemcpyAsync(idx->ws_q.p, q, sizeof(float) * (size_t)B * dim, hipMemcpyDefault, s));
        // the quantisation the searches use: both int8 levels and both error terms
        HIP_TRY(orr::launch_i8_queries(idx->ws_q.as<float>(), B, dim, idx->ws_q8.p, idx->ws_q8s1.as<float>(), idx->ws_q8err.as<double>(), s,
                                       idx->ws_q8err.as<double>() + B));
        if (out_s1) HIP_TRY(hipMemcpyAsync(out_s1, idx->ws_q8s1.p, sizeof(float) * (size_t)B, hipMemcpyDefault, s));
        if (out_err2) HIP_TRY(hipMemcpyAsync(out_err2, idx->ws_q8err.p, sizeof(double) * (size_t)B, hipMemcpyDefault, s));
        if (out_err2_level1) HIP_TRY(hipMemcpyAsync(out_err2_level1, idx->ws_q8err.as<double>() + B, sizeof(double) * (size_t)B, hipMemcpyDefault, s));
        if (out_iq2) HIP_TRY(hipMemcpyAsync(out_iq2, static_cast<const int8_t *>(idx->ws_q8.p) + (size_t)B * dim, (size_t)B * dim, hipMemcpyDefault, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return ORR_OK;
}

int orr_index_screen_i8_stream_dots(orr_index *idx, int32_t B, int32_t dim, const float *q, int32_t unit16, int32_t *out_dots)
{
    if (!idx || !q || !out_dots || B <= 0 || B > orr::kMaxI8ScreenQ) return fail(ORR_EINVAL, "orr_index_screen_i8_stream_dots: bad argument (1..4 queries)");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_screen_i8_stream_dots: the index is not sealed");
    if (dim != idx->dim || dim <= 0 || dim % 128 != 0) return fail(ORR_EINVAL, "orr_index_screen_i8_stream_dots: dim must equal the index dimension and be a multiple of 128");
    if (unit16 && dim % 1024 != 0) return fail(ORR_EINVAL, "orr_index_screen_i8_stream_dots: the 16-row-unit form needs dim % 1024 == 0");
    if (idx->n_rows <= 0) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    ORR_TRY(ensure_i8_shadow(idx));
    if (!idx->i8_ready) return fail(ORR_ENOMEM, "orr_index_screen_i8_stream_dots: the int8 shadow does not fit in device memory");
    hipStream_t s = idx->stream;
    const size_t n = (size_t)idx->n_rows, bytes = sizeof(int32_t) * 2 * (size_t)B * n;
    ORR_TRY(idx->ws_q.reserve(sizeof(float) * (size_t)B * dim));
    ORR_TRY(idx->ws_q8.reserve(2 * (size_t)B * dim));
    ORR_TRY(idx->ws_q8s1.reserve(sizeof(float) * (size_t)B));
    ORR_TRY(idx->ws_q8err.reserve(2 * sizeof(double) * (size_t)B));
    ORR_TRY(idx->ws_dotf.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(idx->ws_q.p, q, sizeof(float) * (size_t)B * dim, hipMemcpyDefault, s));
    HIP_TRY(orr::launch_i8_queries(idx->ws_q.as<float>(), B, dim, idx->ws_q8.p, idx->ws_q8s1.as<float>(), idx->ws_q8err.as<double>(), s,
                                   idx->ws_q8err.as<double>() + B));
    HIP_TRY(hipMemsetAsync(idx->ws_dotf.p, 0xAB, bytes, s));                 // (an element the kernel never writes shows up as 0xABABABAB)
    {
        Timed t(idx, unit16 ? "screen_gemv_i8_dots_u16" : "screen_gemv_i8_dots_u128", 1.0 * (double)n * dim + 2.0 * (double)B * dim + 8.0 * (double)B * (double)n);
        HIP_TRY(orr::launch_screen_gemv_i8_dots(idx->ws_q8.p, B, idx->emb_i8.p, idx->n_rows, dim, idx->ws_dotf.as<int32_t>(), unit16 != 0, s));
    }
    HIP_TRY(hipMemcpyAsync(out_dots, idx->ws_dotf.p, bytes, hipMemcpyDefault, s));
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(idx);
    return ORR_OK;
}

int orr_index_pass_dots(orr_index *idx, int32_t kernel, int32_t B, int32_t dim, const float *q, float *out)
{
    if (!idx || !q || !out || B <= 0 || kernel < 0 || kernel > 1) return fail(ORR_EINVAL, "orr_index_pass_dots: bad argument");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_pass_dots: the index is not sealed");
    if (dim != idx->dim || dim <= 0 || dim % 64 != 0) return fail(ORR_EINVAL, "orr_index_pass_dots: dim must equal the index dimension and be a multiple of 64");
    if (idx->n_rows <= 0) return ORR_OK;
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    const int64_t n = idx->n_rows;
    ORR_TRY(idx->ws_q.reserve(sizeof(float) * (size_t)B * dim));
    ORR_TRY(idx->ws_dotf.reserve(sizeof(float) * (size_t)B * (size_t)n));
    HIP_TRY(hipMemcpyAsync(idx->ws_q.p, q, sizeof(float) * (size_t)B * dim, hipMemcpyDefault, s));
    if (kernel == 0) {
        for (int32_t b0 = 0; b0 < B; b0 += 32) {                               // groups of 32, as the pass sends them (launch_numerators)
            const int32_t nq = std::min<int32_t>(32, B - b0);
            Timed t(idx, "gemv_mfma", 4.0 * (double)n * dim + 4.0 * (double)nq * dim + 4.0 * (double)nq * (double)n);
            HIP_TRY(orr::launch_gemv_mfma(idx->ws_q.as<float>() + (size_t)b0 * dim, nq, idx->d_emb, n, dim, idx->ws_dotf.as<float>() + (size_t)b0 * n, n, s));
        }
    } else {
        ORR_TRY(idx->ws_qsplit.reserve(sizeof(float) * (size_t)B * dim));
        HIP_TRY(orr::launch_split_queries(idx->ws_q.as<float>(), B, dim, idx->ws_qsplit.p, s));
        Timed t(idx, "gemm_dot_bf16x3", 4.0 * (double)n * dim + 4.0 * (double)B * dim + 4.0 * (double)B * (double)n);
        HIP_TRY(orr::launch_gemm_dot_bf16x3(idx->ws_qsplit.p, B, idx->d_emb, 0, n, dim, idx->ws_dotf.as<float>(), n, nullptr, 3, s));
    }
    HIP_TRY(hipMemcpyAsync(out, idx->ws_dotf.p, sizeof(float) * (size_t)B * (size_t)n, hipMemcpyDefault, s));
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(idx);
    return ORR_OK;
}

int orr_index_capture_screen(orr_index *idx, int32_t enabled)
{
    if (!idx) return fail(ORR_EINVAL, "orr_index_capture_screen: null index");
    LanePool::Exclusive all(pool_of(idx));             // no search in flight on any lane while the switch moves
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_capture_screen: the index is not sealed");
    ScreenCapture &c = idx->capture;
    if (enabled) {
        c.have = false;
        c.floor_key.clear(); c.L.clear(); c.cnt.clear(); c.buf.clear();
    }
    c.armed.store(enabled ? 1 : 0, std::memory_order_relaxed);
    return ORR_OK;
}

int orr_index_captured_screen(orr_index *idx, orr_screen_capture *info, int32_t B, uint32_t cap, uint64_t *out_floor_key, double *out_L,
                              uint32_t *out_cnt, uint64_t *out_key, uint32_t *out_pos)
{
    if (!info) return fail(ORR_EINVAL, "orr_index_captured_screen: info is NULL");
    const int given = (out_floor_key != nullptr) + (out_L != nullptr) + (out_cnt != nullptr) + (out_key != nullptr) + (out_pos != nullptr);
    if (given != 0 && given != 5) return fail(ORR_EINVAL, "orr_index_captured_screen: give all five arrays or none");
    if (given && (B <= 0 || cap == 0)) return fail(ORR_EINVAL, "orr_index_captured_screen: arrays given with B <= 0 or cap == 0");
    if (!idx) return fail(ORR_EINVAL, "orr_index_captured_screen: null index");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_captured_screen: the index is not sealed");
    const ScreenCapture &c = idx->capture;
    if (!c.have) return fail(ORR_ESTATE, "orr_index_captured_screen: nothing was captured since the handle was armed");
    if (given && (B != c.info.B || cap != c.info.cap)) return fail(ORR_EINVAL, "orr_index_captured_screen: B or cap differ from the capture's");
    *info = c.info;
    if (!given) return ORR_OK;
    const size_t nb = (size_t)c.info.B, kc = (size_t)c.info.cap;
    for (size_t b = 0; b < nb; ++b) {
        out_floor_key[b] = c.floor_key[b];
        out_L[b] = c.L[b];
        out_cnt[b] = c.cnt[b];
        const size_t filled = std::min<size_t>(c.cnt[b], kc);
        for (size_t i = 0; i < filled; ++i) {
            out_key[b * kc + i] = c.buf[b * kc + i].key;
            out_pos[b * kc + i] = c.buf[b * kc + i].pos;
        }
    }
    return ORR_OK;
}

int orr_index_set_profiling(orr_index *idx, int32_t enabled)
{
    if (!idx) return fail(ORR_EINVAL, "null index");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    const int level = enabled == 2 ? 2 : (enabled != 0 ? 1 : 0);
    for_each_lane(idx, [&](orr_index *x) { x->profiling = level; x->stats.clear(); });
    return ORR_OK;
}

int orr_index_kernel_stats(orr_index *idx, orr_kernel_stat *out, int32_t cap)
{
    if (!idx) return fail(ORR_EINVAL, "null index");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    std::vector<KernelStat> sum;                        // every lane's launches, by kernel name
    for_each_lane(idx, [&](orr_index *l) {
        for (const KernelStat &ks : l->stats) {
            size_t i = 0;
            while (i < sum.size() && sum[i].name != ks.name) ++i;
            if (i == sum.size()) { sum.push_back(ks); continue; }
            sum[i].launches += ks.launches; sum[i].total_ms += ks.total_ms; sum[i].algo_bytes += ks.algo_bytes;
        }
    });
    const int32_t n = (int32_t)sum.size();
    for (int32_t i = 0; i < n && i < cap && out; ++i) {
        memset(&out[i], 0, sizeof(orr_kernel_stat));
        strncpy(out[i].name, sum[(size_t)i].name.c_str(), sizeof(out[i].name) - 1);
        out[i].launches = sum[(size_t)i].launches;
        out[i].total_ms = sum[(size_t)i].total_ms;
        out[i].algo_bytes = sum[(size_t)i].algo_bytes;
    }
    return n;
}

}  // extern "C"

namespace {

struct BatchArgs {
    int32_t B, dim;
    const float *q;
    const uint8_t *terms_utf8;
    const uint32_t *term_off;
    const uint32_t *query_term_off;
    int64_t now_ticks;
    int64_t candidate_limit;
    int32_t topk = 10;             // the caller's k (two-stage floor); kprime is passed separately
    bool force_exact = false;      // skip the MFMA candidate pass (escalation after a failed certificate)
    bool no_fuse = false;          // keep the batched pass unfused (retry after a candidate-buffer overflow)
    const double *norms_host = nullptr; // exact normA of every query, already computed by the caller (orr_cluster: once for all shards)
    orr_candidate *out_dev = nullptr;   // orr_search_shard with a device-resident `out`: the kernels write the records there
    int64_t *out_keys = nullptr;        // orr_search_batch_diverse: [B][max(1, topk)] of the CALL's numbering, each result's order_key beside out_rows
};

const orr_index *owner_of(const orr_index *idx) { return idx->parent ? idx->parent : idx; }

int check_batch(const orr_index *idx, const BatchArgs &a, const char *fn)
{
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    if (!idx->sealed) return fail(ORR_ESTATE, "%s: index is not sealed", fn);
    if (a.B <= 0) return fail(ORR_EINVAL, "%s: batch size must be positive", fn);
    if (a.dim < 0) return fail(ORR_EINVAL, "%s: negative query dimension", fn);
    if (a.dim > 0 && !a.q) return fail(ORR_EINVAL, "%s: q is NULL with dim %d", fn, a.dim);
    if (!a.query_term_off) return fail(ORR_EINVAL, "%s: query_term_off is required", fn);
    return ORR_OK;
}

// Rows of this shard that take part: the global candidate prefix clipped to the shard.
// Deleted rows do not count: the prefix ends behind the shard's local_live-th live row.
int64_t participating_rows(const orr_index *idx, int64_t candidate_limit)
{
    const std::vector<int64_t> &dead = owner_of(idx)->dead;
    return cper_key::prefix_rows(candidate_limit, idx->row_base, idx->dead_before, idx->n_rows, dead.data(), dead.size());
}

bool is_device_pointer(const void *p)
{
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();            // plain malloc'd memory: not known to the runtime
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}

// Rows of the sampled prefix of the two-stage pass, in selection segments (4096 rows each).  A larger
// sample gives a tighter floor (fewer survivors to re-score) and costs a larger ranking pass; the survivors
// of one query are about 2 k n / sample when scores are continuous (far fewer when keyword matches make
// them step-like), and they must stay well inside the 8192-entry buffers: k n / 2000 rows.  Measured (full
// hybrid scores): 1M rows x 1024 queries, 4 / 8 / 16 segments = 9.7 / 10.4 / 11.3 ms per batch; 12.5M rows x
// 1024 queries, 4 / 16 / 64 segments = 84.3 / 86.8 / 95.4 ms; the re-score stays below 0.4 ms throughout.
// The streaming form (1..8 queries) re-scores in parallel waves whose time does not grow with the number
// of survivors, so it goes down to two segments.
// boost (1..16, orr_index::sample_boost): scores without steps (cosine-only queries: config C4) leave 10..50 times as
// many survivors as hybrid ones, because the int8 bound is then comparable to the spacing of the scores around the
// floor; the index doubles the sample while the measured survivors per query stay above 4096 and halves it again
// below 512 (12.5M rows, 256 cosine-only queries, k' = 32: 16,000 survivors per query and 10 ms of exact re-scoring
// with the default sample of 200k rows against 14 ms for the screen itself; four times the sample, a quarter of both).
static int32_t sample_segments(int32_t n_seg_all, int64_t n, int32_t k, bool small_batch, int boost)
{
    const int64_t rows = (int64_t)std::max<int32_t>(1, k) * n / 2000 * std::max(1, boost);
    const int64_t segs = (rows + orr::kSelSegRows - 1) / orr::kSelSegRows;
    const int64_t most = std::min<int64_t>(64 * (int64_t)std::max(1, boost), std::max<int64_t>(n_seg_all / 8, 4));   // never more than an eighth of the rows
    return (int32_t)std::min<int64_t>(most, std::max<int64_t>(small_batch ? 2 : 4, segs));
}

// ORR_HOST_TIMING=1: where the host side of a search spends its time, printed to stderr every 64 calls (diagnostic,
// one searching thread).
struct HostTiming {
    bool on = getenv("ORR_HOST_TIMING") != nullptr;
    double acc[8] = {0};
    int64_t calls = 0;
    std::chrono::steady_clock::time_point last;
    void start() { if (on) last = std::chrono::steady_clock::now(); }
    void mark(int i)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        acc[i] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
    void done()
    {
        if (!on || ++calls % 64 != 0) return;
        fprintf(stderr, "[orr host ms/call] query_setup+cos_launch %.3f | keyword_prep+launch %.3f | norms+consts %.3f | select_launches %.3f | "
                        "wait_gpu %.3f | finish %.3f\n", acc[0] / 64, acc[1] / 64, acc[2] / 64, acc[3] / 64, acc[4] / 64, acc[5] / 64);
        for (double &x : acc) x = 0;
    }
};
thread_local HostTiming g_ht;          // per searching thread: lanes (views) and cluster workers each time their own calls

// ---- K3, the keyword side of one pass, on its own stream (with the int8 prefix the main stream has little to do before it
// needs the bitmaps, so this chain is the critical path of a batch): distinct terms -> vocabulary scan -> (term, token) hits ->
// per distinct term a row bitmap: a stored token bitmap where the term's only hit has one (ensure_token_bitmaps), else its
// posting lists OR-ed into the batch's own bitmaps (orr_token_index.cpp: why this equals RecallSearchService.cs:111).
struct KwSide {
    orr::KwView view{nullptr, 0, nullptr, nullptr, nullptr};
    size_t bm_bytes = 0, bm_clean_before = 0;     // the batch's own bitmaps: bytes used, bytes known to be zero on entry
    bool overflow_possible = false;               // the hit list may have been too short (checked behind the pass)
    uint32_t max_hits = 0;
    const uint8_t *alias = nullptr;               // per distinct term: its bitmap is a stored token bitmap (device; null without a token store)
};

// ORR_VOCAB_LOOKUP=0|1 forces the short tokens' form, ORR_VOCAB_MID=0 sends the tokens of 17..32 bytes through the wave-per-token
// scan like the longer ones (A/B): read once, at the first chain; a call's own overrides (orr_index_keyword_bitmaps) go first
struct KwEnv {
    int lookup;        // -1 unset
    bool mid_off;
};
static int env_switch(const char *v) { return v ? atoi(v) : -1; }
static const KwEnv &kw_env()
{
    static const KwEnv e{env_switch(getenv("ORR_VOCAB_LOOKUP")), env_switch(getenv("ORR_VOCAB_MID")) == 0};
    return e;
}

// One chain's working set: what the plan decided (orr_keyword_plan.h) and what a stage hands to the ones behind it.
struct KwWork {
    hipStream_t k = nullptr;
    uint32_t n_terms_total = 0, TT = 0;
    bool lookup = false;                          // the short tokens' form
    keyword::MetaLayout lay{};
    int64_t V = 0, VL = 0, n_mid = 0, words = 0;  // tokens, the long ones, of those one lane per token; words of a bitmap
    keyword::HitList hits{0, false};
    KwVouchers held;                              // what the last chain on this lane left clean
    size_t bm_bytes = 0, bm_clean = 0;            // the batch's own bitmaps: bytes used, leading bytes that are zero already
    bool counters_clean = false;
    uint8_t *dm = nullptr;                        // the image on the device
    const int64_t *term_word_off = nullptr;       // the alias stage's, where the shard stores token bitmaps
    const uint8_t *skip = nullptr;
};

// 1. the distinct terms, the short tokens' form, the image in pinned memory
static int kw_plan_and_fill(orr_index *idx, const BatchArgs &a, const std::vector<uint32_t> &qoff, KwWork &w)
{
    keyword::Distinct d;
    const int64_t bad = keyword::distinct_terms(a.terms_utf8, a.term_off, qoff.data(), a.B, d);
    if (bad >= 0) return fail(ORR_EINVAL, "term_off is not monotone at term %u", (uint32_t)bad);
    w.TT = (uint32_t)d.terms.size();
    w.lookup = keyword::short_form(w.TT, idx->n_tokens, idx->kw_force_form, kw_env().lookup);
    idx->kw_form_ran = w.lookup ? 1 : 0;
    w.lay = keyword::layout_of(w.TT, w.n_terms_total, a.B, d.pool_bytes, w.lookup);
    ORR_TRY(idx->pin_meta.reserve(w.lay.meta_bytes));
    ORR_TRY(idx->ws_meta.reserve(w.lay.meta_bytes));
    keyword::fill_meta(idx->pin_meta.as<uint8_t>(), w.lay, d, w.lookup);
    return ORR_OK;
}

// 2. the workspaces.  The term bitmaps must start out zero.  Every search clears what it used again when it is done (behind its
// last kernel, while the host finishes the batch), so the next one only clears what lies beyond: the memset (270 MB at 1024
// queries x 1M rows) leaves the critical path of the keyword chain.  The vouchers are withdrawn here -- until this chain's
// caller has cleaned up after it -- and compared behind the reserve: the buffer may have moved.
static int kw_reserve(orr_index *idx, KwWork &w)
{
    w.V = idx->n_tokens;
    w.words = keyword::words_per_term(idx->n_rows);
    w.hits = keyword::hit_list(w.V, w.TT, idx->kw_hits_cap);
    ORR_TRY(ensure_vlong(idx));
    ORR_TRY(ensure_token_bitmaps(idx));
    w.VL = idx->n_vlong;
    w.n_mid = keyword::mid_tokens(idx->n_vmid, w.VL, idx->kw_force_mid, kw_env().mid_off);
    w.bm_bytes = sizeof(uint32_t) * (size_t)w.TT * (size_t)w.words;
    ORR_TRY(idx->ws_vmatch.reserve(sizeof(uint16_t) * (size_t)w.TT * (size_t)std::max<int64_t>(w.VL, 1)));
    ORR_TRY(idx->ws_bitmaps.reserve(w.bm_bytes));
    w.held = idx->kw_clean.withdraw();
    w.bm_clean = w.held.bitmaps_of == idx->ws_bitmaps.p ? w.held.bitmaps : 0;
    ORR_TRY(idx->ws_hits.reserve(sizeof(orr::KwHit) * (size_t)w.hits.max_hits));
    ORR_TRY(idx->ws_counter.reserve(sizeof(unsigned long long)));
    ORR_TRY(idx->pin_kwcnt.reserve(sizeof(unsigned long long)));
    // (the chain's counters were zeroed behind the last search on this stream, unless this is the first one or they moved)
    w.counters_clean = w.held.counters && w.held.counters_of[0] == idx->ws_counter.p;
    return ORR_OK;
}

// 3. the image goes up in one copy; the hit counter starts at zero, on the device and in pinned memory
static int kw_upload(orr_index *idx, KwWork &w)
{
    *idx->pin_kwcnt.as<unsigned long long>() = 0ull;
    w.dm = idx->ws_meta.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(w.dm, idx->pin_meta.as<uint8_t>(), w.lay.meta_bytes, hipMemcpyHostToDevice, w.k));
    if (!w.counters_clean) HIP_TRY(hipMemsetAsync(idx->ws_counter.p, 0, sizeof(unsigned long long), w.k));
    return ORR_OK;
}

// 4. tokens of at most 16 bytes: one lane per token against every distinct term, hits reserved in place; where tokens x terms
// is large the terms are looked up (sorted by first dword) instead of compared one by one
static int kw_match_short(orr_index *idx, const KwWork &w)
{
    const orr::MatchTerm *terms = reinterpret_cast<const orr::MatchTerm *>(w.dm + w.lay.match);
    Timed t(idx, "vocab_match", 0.0, w.k);
    if (w.lookup) {
        const uint32_t *lk = reinterpret_cast<const uint32_t *>(w.dm + w.lay.lk);
        HIP_TRY(orr::launch_vocab_match_lookup(idx->d_vpool, idx->d_vstart, idx->d_vlen, w.V, terms, lk, lk + keyword::kLkHead,
                                               lk + keyword::kLkHead + w.TT, reinterpret_cast<const uint32_t *>(w.dm + w.lay.bloom), idx->d_post_off,
                                               idx->ws_counter.as<unsigned long long>(), idx->ws_hits.as<orr::KwHit>(), w.hits.max_hits, w.k));
    } else {
        HIP_TRY(orr::launch_vocab_match_short(idx->d_vpool, idx->d_vstart, idx->d_vlen, w.V, terms, (int32_t)w.TT, idx->d_post_off,
                                              idx->ws_counter.as<unsigned long long>(), idx->ws_hits.as<orr::KwHit>(), w.hits.max_hits, w.k));
    }
    return ORR_OK;
}

// 5. the longer tokens: those of 17..32 bytes (the front of their list) one lane per token as well; for the rest every distinct
// term is its own 1-term "query" of the wave-per-token scan
static int kw_match_long(orr_index *idx, const KwWork &w)
{
    const int32_t TT = (int32_t)w.TT;
    const int64_t n_mid = w.n_mid, VS = w.VL - n_mid;
    if (n_mid > 0) {
        Timed t(idx, "vocab_match_mid", 0.0, w.k);
        HIP_TRY(orr::launch_vocab_match_mid(idx->d_vpool, idx->vlong_start.as<uint64_t>(), idx->vlong_len.as<uint32_t>(),
                                            idx->vlong_id.as<uint32_t>(), n_mid, reinterpret_cast<const orr::MatchTerm8 *>(w.dm + w.lay.match8),
                                            TT, idx->d_post_off, idx->ws_counter.as<unsigned long long>(),
                                            idx->ws_hits.as<orr::KwHit>(), w.hits.max_hits, w.k));
    }
    if (VS <= 0) return ORR_OK;
    {
        Timed t(idx, "vocab_scan", 0.0, w.k);
        HIP_TRY(orr::launch_vocab_scan(idx->d_vpool, idx->vlong_start.as<uint64_t>() + n_mid, idx->vlong_len.as<uint32_t>() + n_mid, VS,
                                       w.dm + w.lay.pool, reinterpret_cast<const orr::ScanTerm *>(w.dm + w.lay.terms), TT,
                                       reinterpret_cast<const uint32_t *>(w.dm + w.lay.iota), idx->ws_vmatch.as<uint16_t>(), w.k));
    }
    Timed t(idx, "vocab_hits", 0.0, w.k);
    HIP_TRY(orr::launch_vocab_hits(idx->ws_vmatch.as<uint16_t>(), VS, TT, idx->vlong_id.as<uint32_t>() + n_mid, idx->d_post_off,
                                   idx->ws_counter.as<unsigned long long>(), idx->ws_hits.as<orr::KwHit>(), w.hits.max_hits, w.k));
    return ORR_OK;
}

// 6. terms whose only hit is a token with a stored bitmap use that bitmap as it is (no expansion, nothing copied)
static int kw_alias(orr_index *idx, KwWork &w)
{
    if (!(idx->n_tok_bm > 0 && idx->tok_bm_words == w.words)) return ORR_OK;
    const size_t TT = w.TT;
    const size_t o_tok = sizeof(uint32_t) * TT, o_off = (2 * o_tok + 7) / 8 * 8, o_alias = o_off + sizeof(int64_t) * TT;
    ORR_TRY(idx->ws_kwalias.reserve(o_alias + TT + 16));
    uint8_t *wa = idx->ws_kwalias.as<uint8_t>();
    if (!(w.counters_clean && w.held.counters_of[1] == idx->ws_kwalias.p))
        HIP_TRY(hipMemsetAsync(wa, 0, o_tok, w.k));              // the hit counts
    const int64_t delta = (int64_t)(idx->tok_bm.as<uint32_t>() - idx->ws_bitmaps.as<uint32_t>());   // words from the batch's bitmaps to the token store
    Timed t(idx, "kw_alias", 0.0, w.k);
    HIP_TRY(orr::launch_kw_alias(idx->ws_hits.as<orr::KwHit>(), idx->ws_counter.as<unsigned long long>(), w.hits.max_hits, (int32_t)TT,
                                 idx->tok_bm_index.as<int32_t>(), delta, w.words, reinterpret_cast<uint32_t *>(wa),
                                 reinterpret_cast<uint32_t *>(wa + o_tok), reinterpret_cast<int64_t *>(wa + o_off), wa + o_alias, w.k));
    w.term_word_off = reinterpret_cast<const int64_t *>(wa + o_off);
    w.skip = wa + o_alias;
    return ORR_OK;
}

// 7. the bitmaps are first written behind this: the clearing behind the last search (on the auxiliary stream) must be done,
// and what lies beyond the cleared part is cleared now.  (A corpus without tokens: nothing is expanded, the bitmaps are read
// all the same.)
static int kw_settle_bitmaps(orr_index *idx, const KwWork &w)
{
    if (idx->kw_clean.clear_in_flight) {
        HIP_TRY(hipStreamWaitEvent(w.k, idx->ev_bm_clean, 0));
        idx->kw_clean.clear_in_flight = false;
    }
    if (w.bm_clean < w.bm_bytes)
        HIP_TRY(hipMemsetAsync(static_cast<uint8_t *>(idx->ws_bitmaps.p) + w.bm_clean, 0, w.bm_bytes - w.bm_clean, w.k));
    return ORR_OK;
}

// 8. the hits' posting lists OR-ed into the bitmaps; the hit count goes to pinned memory (statistics, and the check of the list)
static int kw_expand(orr_index *idx, const KwWork &w)
{
    Timed t(idx, "expand_hits", 0.0, w.k);
    HIP_TRY(orr::launch_expand_hits(idx->ws_hits.as<orr::KwHit>(), idx->ws_counter.as<unsigned long long>(), w.hits.max_hits,
                                    idx->d_post_rows, idx->ws_bitmaps.as<uint32_t>(), w.words, w.k,
                                    idx->pin_kwcnt.as<unsigned long long>(), w.skip));
    return ORR_OK;
}

int launch_keyword_side(orr_index *idx, const BatchArgs &a, const std::vector<uint32_t> &qoff, KwSide &out)
{
    KwWork w;
    w.k = idx->stream_kw;
    w.n_terms_total = qoff[(size_t)a.B] - qoff[0];
    if (w.n_terms_total == 0) return ORR_OK;
    ORR_TRY(kw_plan_and_fill(idx, a, qoff, w));
    ORR_TRY(kw_reserve(idx, w));
    out.bm_bytes = w.bm_bytes;
    out.bm_clean_before = w.bm_clean;
    ORR_TRY(kw_upload(idx, w));
    if (w.V > 0) {
        ORR_TRY(kw_match_short(idx, w));
        ORR_TRY(kw_match_long(idx, w));
        ORR_TRY(kw_alias(idx, w));
    }
    ORR_TRY(kw_settle_bitmaps(idx, w));
    if (w.V > 0) ORR_TRY(kw_expand(idx, w));
    // 9. the main stream joins behind this event
    HIP_TRY(hipEventRecord(idx->ev_kw_done, w.k));
    out.view.bitmaps = idx->ws_bitmaps.as<uint32_t>();
    out.view.words_per_term = w.words;
    out.view.q_term_idx = reinterpret_cast<const uint32_t *>(w.dm + w.lay.qmeta);
    out.view.q_term_off = out.view.q_term_idx + w.n_terms_total;
    out.view.term_word_off = w.term_word_off;
    out.alias = w.skip;
    out.overflow_possible = w.hits.overflow_possible;
    out.max_hits = w.hits.max_hits;
    return ORR_OK;
}

// Generic path for large k (topK beyond the 64 entries a wave keeps): every score of a query, a stable descending radix sort
// (hipCUB), the first k' rows as records -- query by query.
int run_large_k(orr_index *idx, const BatchArgs &a, int32_t kprime, int64_t n, const double *d_dot, const orr::KwView &kw,
                const orr::QueryConst *qc, orr_candidate *d_cand, hipStream_t s)
{
    const int32_t B = a.B;
    // generic large-k path: full stable sort of every score, query by query
    ORR_TRY(idx->ws_keys_a.reserve(sizeof(unsigned long long) * (size_t)n));
    ORR_TRY(idx->ws_keys_b.reserve(sizeof(unsigned long long) * (size_t)n));
    ORR_TRY(idx->ws_vals_a.reserve(sizeof(uint32_t) * (size_t)n));
    ORR_TRY(idx->ws_vals_b.reserve(sizeof(uint32_t) * (size_t)n));
    size_t tmp_bytes = 0;
    HIP_TRY(orr::sort_pairs_desc(nullptr, tmp_bytes, idx->ws_keys_a.as<unsigned long long>(),
                                 idx->ws_keys_b.as<unsigned long long>(), idx->ws_vals_a.as<uint32_t>(),
                                 idx->ws_vals_b.as<uint32_t>(), n, s));
    ORR_TRY(idx->ws_sort_tmp.reserve(tmp_bytes));
    for (int32_t b = 0; b < B; ++b) {
        const double *dq = d_dot ? d_dot + (size_t)b * n : nullptr;
        {
            Timed t(idx, "score_keys", (double)n * 36.0);
            HIP_TRY(orr::launch_score_keys(dq, idx->d_norm_b, idx->d_created, kw, b, qc[b], a.now_ticks, n,
                                           idx->ws_keys_a.as<unsigned long long>(), idx->ws_vals_a.as<uint32_t>(), s));
        }
        {
            Timed t(idx, "radix_sort_desc", (double)n * 12.0 * 2.0 * 8.0);
            size_t tb = idx->ws_sort_tmp.cap;
            HIP_TRY(orr::sort_pairs_desc(idx->ws_sort_tmp.p, tb, idx->ws_keys_a.as<unsigned long long>(),
                                         idx->ws_keys_b.as<unsigned long long>(), idx->ws_vals_a.as<uint32_t>(),
                                         idx->ws_vals_b.as<uint32_t>(), n, s));
        }
        HIP_TRY(orr::launch_records_from_sorted(idx->ws_keys_b.as<unsigned long long>(), idx->ws_vals_b.as<uint32_t>(),
                                                kprime, n, idx->row_base, d_dot, n, idx->d_norm_b, idx->d_created,
                                                idx->d_row_ids, kw, b, 1, d_cand + (size_t)b * (kprime + 1), s));
    }
    return ORR_OK;
}

// up to this many queries (a grid dimension) the tail of the two-stage pass is finish_survivors: one launch, two from 64 queries
// on (12.5M rows x 1024 queries: 0.26 ms against 0.70 for the four separate kernels below, which remain for dim % 256 != 0)
constexpr int kFinishFusedMaxB = 65535;
constexpr int kRetryPass = 1;          // run_shard_once: a workspace was too small and has been enlarged; the same pass again

// ---- One shard pass: a plan settled up front (plan_pass), then the stages that run it (run_shard_once).

// Error of the approximate dot against the reference sum, relative to sum|q_k e_k| (<= |q||e| by Cauchy-Schwarz, which turns
// it into a bound on the cosine).  The matrix cores' internal summation order and rounding mode are not documented, so every
// addition (and every fp32 product) is charged one full unit in the last place, 2^-23, of a partial sum that never exceeds
// sum|terms|:
//   f32 MFMA    D products + D additions                      -> (2 D + 2) 2^-23
//   split bf16  3 D additions of exact products, plus the dropped lo*lo and the second-order
//               residuals of the split (u = 2^-8 per bf16 rounding) -> 3.1 u^2 + 3.06 D 2^-23
//   plain bf16  (1 + u)^2 - 1 per product, D additions charged 2^-23 each -> 2^-7 (1 + 2^-9) + 1.02 D 2^-23
// The int8 forms add their per-pair bound inside the kernels: the keys they leave are already lower bounds (kEpsI8).
// All three charge the reference's fp32 products a RELATIVE error, which holds while those products are normal numbers.  The
// int8 forms hand rows with 0 < normB < 2^-96 and queries with 0 < max|q| < 2^-48 to the exact pass (orr_screen.hip,
// kI8MinNormB).  These three have no per-row never-drop value: a host-resident batch that holds such a query takes the exact
// pass (plan_form, has_tiny_query; without it the bf16 shadow and the in-kernel bf16 conversion lose a winner whose products
// are subnormal, tests/test_gpu_screen_bounds.py); such a query in device memory is marked from its norm where the device or
// the host forms it (orr::kQueryKeepAll, launch_consts): every pair of it is kept, the query comes back uncertified and the
// ladder ends in the exact pass.  Rows that small stay out of contract on these three forms.
// At the large end the contract reaches as far as the reference's own arithmetic does: while every fp32 square and product is
// finite (|q_k|, |e_k| up to 1.8e19) the norms and the reference's double sums are ordinary numbers, but the fp32 sums of all
// three forms overflow to +inf or -inf -- a relative bound says nothing about those.  Such a pair (a dot that is not finite
// beside finite positive norms: dot_overflowed, and the float epilogues' own tests) is never cut: a ranking keeps it under
// the all-ones key for the exact re-score, a floor takes nothing from it, and a list that such pairs fill reports a cut-off of
// +inf, which leaves the query uncertified (tests/test_gpu_overflowing_sums.py).  Rows and queries with a NaN or an infinite
// coordinate, or with a square that overflows (1e25), have a norm that is NaN or infinite and keep the lowest key.
constexpr double kU23 = 1.1920928955078125e-07, kU16 = 1.52587890625e-05;
constexpr double kEpsI8 = 1e-12;
double cosine_bound(double eps_cos) { return 0.7 * 1.01 * eps_cos + 1e-12; }
double eps_f32_mfma(int32_t D) { return cosine_bound((2.0 * (double)D + 2.0) * kU23); }
double eps_split_bf16(int32_t D) { return cosine_bound(3.1 * kU16 + 3.06 * (double)D * kU23); }
double eps_plain_bf16(int32_t D) { return cosine_bound(0.0078125 * (1.0 + 0.001953125) + 1.02 * (double)D * kU23); }

// The form of one shard pass: which launches a batch gets (Timed names; DESIGN.md §10 has the table).
enum class PassForm {
    Empty,           // no participating row: trailer records only
    Exact,           // dot_exact (or no vector side), row_consts, fuse_select, select_final
    StreamMfma,      // gemv_mfma over all rows, then as Exact, then rescore_exact
    SplitAll,        // gemm_dot_bf16x3 over all rows, then as Exact, then rescore_exact
    SplitFused,      // gemm_dot_bf16x3 over a sampled prefix -> floor -> gemm_dot_bf16x3_fused over the rest, rescore_exact
    TwoStageGemm,    // prefix -> floor -> screening GEMM over all rows into survivors' buffers -> exact tail
    TwoStageStream,  // 1..8 queries: the streaming screen over the prefix -> floor, over all rows -> survivors -> exact tail
    LargeK,          // k' beyond a selection list: run_large_k
};

// The screen of the two-stage forms over all rows, in the order of orr_search_stats.pass_mode: screen_i8_fused (K2j) in row
// ranges, screen_gemv_i8 (K2i), screen_gemv_bf16 (K2g), screen_bf16_fused (K2c), gemm_dot_bf16x1_fused (fp32 rows converted).
enum class Screen { None, I8Ranges, GemvI8, GemvBf16, Bf16Shadow, Bf16x1 };

struct PassPlan {
    PassForm form = PassForm::Exact;
    Screen screen = Screen::None;
    bool use_cos = false;
    bool use_mfma = false;          // records carry no dot yet: filled in exactly on the device (an empty shard: the batch's choice)
    bool q_on_device = false;       // the caller's query vectors are device memory
    bool dev_norms = false;         // the queries' exact norms are computed on the device
    bool prefix_i8 = false;         // the sampled prefix goes through the int8 screening GEMM: its keys are lower bounds
    bool split_queries = false;     // the hi/lo bf16 split of the queries (launch_split_queries)
    bool batched_score = false;     // per-row pieces once per batch
    bool rowc_inline = false;       // the int8 stream forms the row constants in its epilogue (one or two uses per row)
    int32_t fused_sample_seg = 0;   // > 0: fused epilogue behind a sampled prefix of that many segments
    int64_t dotf_rows = 0;          // columns of the fp32 dots
    int n_ranges = 1;               // row ranges of the int8 screening GEMM: [range_row[r], range_row[r + 1])
    int64_t range_row[17] = {};
    int32_t count_bits = 0;         // FusedEpilogue::count_bits
    int prefix_floor_form = 0;      // fuse_select floor_only of the sampled prefix
    double approx_eps = 0.0;        // bound of the approximate scores of the batched pass (and of the two-stage prefix)
    double eps1 = 0.0;              // two-stage: bound of the screen over all rows (0: added inside the kernel)
    bool masked = false;            // the screen runs under a scope mask (run_masked_pass): no prefix, the floor from an in-scope sample
    bool grouped = false;           // ... under the masks of several groups at once (a masked pass with a GroupScopes)
    bool keep_tiny = false;         // device-resident queries through a float form: orr::kQueryKeepAll is set by the norm (launch_consts)

    bool two_stage() const {   // the pass keeps survivors in per-query buffers (idx->h_survivors holds their counts)
        return form == PassForm::TwoStageGemm || form == PassForm::TwoStageStream;
    }
    bool stream() const { return form == PassForm::TwoStageStream; }
    double plane_bytes_per_row(int32_t B) const { return (count_bits == 2 ? 8.0 : 16.0) * (double)((B + 31) / 32); }   // count words
    bool fused() const { return fused_sample_seg > 0; }
    int pass_mode() const { static constexpr int kMode[] = {0, 1, 1, 2, 2, 3}; return grouped ? 6 : masked ? 5 : kMode[(int)screen]; }   // orr_search_stats
};

// Whether a host-resident batch holds a query whose largest coordinate is positive and below 2^-48: its products with the rows
// are subnormal in fp32, where the relative product error that cosine_bound charges does not hold (see the eps table above).
static bool has_tiny_query(const float *q, int32_t B, int32_t D)
{
    for (int32_t b = 0; b < B; ++b) {
        float mx = 0.f;
        for (int32_t k = 0; k < D; ++k) mx = std::max(mx, std::fabs(q[(size_t)b * D + k]));
        if (mx > 0.f && mx < 0x1p-48f) return true;
    }
    return false;
}

// Decides the form of one pass and what it derives, building the shadows it reads.
int plan_form(orr_index *idx, const BatchArgs &a, int32_t kprime, int64_t n, const std::vector<uint32_t> &qoff, PassPlan &p)
{
    const int32_t B = a.B, D = idx->dim;
    const int32_t n_seg_all = (int32_t)((n + orr::kSelSegRows - 1) / orr::kSelSegRows);
    const bool small_k = kprime <= orr::kSelWidth;
    const bool floor_fits = !a.no_fuse && n_seg_all >= 48 && std::max<int32_t>(1, a.topk) <= orr::kSelWidth;
    p = PassPlan{};
    p.use_cos = a.dim > 0 && a.dim == D;
    p.q_on_device = p.use_cos && is_device_pointer(a.q);
    // the forms without the int8 shadow's per-pair bound have no way to keep such a query's pairs: the exact pass takes the batch
    const bool force_exact = a.force_exact || (p.use_cos && (idx->opt_two_stage != 1 || D % 128 != 0) && !p.q_on_device &&
                                               has_tiny_query(a.q, B, D));
    // 1..8 queries over a large shard with a shadow in place: the streaming form of the two-stage pass
    // (stream over a sampled prefix -> floor, stream over all rows -> survivors, exact re-score)
    bool stream = false, stream_i8 = false;
    if (p.use_cos && !force_exact && idx->opt_two_stage == 1 && D % 64 == 0 && small_k && floor_fits && B <= orr::kMaxGemvScreenQ) {
        ORR_TRY(ensure_i8_shadow(idx));
        stream_i8 = idx->i8_ready;
        if (!stream_i8) ORR_TRY(ensure_shadow(idx));
        stream = stream_i8 || idx->shadow_ready;
        // 5..8 queries on the int8 shadow: the screening GEMM with one live query tile is HBM-bound as well and
        // reads the rows once, the stream would need two launches (1M x 3072: 8 queries 1.39 -> 0.97 ms)
        if (stream_i8 && B > orr::kMaxI8ScreenQ) stream = stream_i8 = false;
    }
    // Batched candidate pass on the matrix cores (K2) + exact re-score (K6) from 5 queries up; below it the HBM-bound exact
    // kernel is as fast and needs no second pass.
    p.use_mfma = p.use_cos && !force_exact && (B >= 5 || stream) && D % 64 == 0 && small_k;
    // Queries that already live on the device get their exact norms there (a handful of queries: the download and the
    // host's pass cost less than the kernel's 3072-step chains).  The generic large-k path scores with host-side constants.
    p.dev_norms = p.q_on_device && small_k && B >= 16 && !a.norms_host;
    p.batched_score = (B >= 4 || stream) && small_k;
    p.dotf_rows = n;
    for (int r = 1; r <= 16; ++r) p.range_row[r] = n;
    if (n == 0) { p.form = PassForm::Empty; return ORR_OK; }
    if (!small_k) { p.form = PassForm::LargeK; return ORR_OK; }
    if (!p.use_mfma) { p.form = PassForm::Exact; return ORR_OK; }
    if (stream) {
        // 1..8 queries: HBM-bound, so no GEMM tile: the streaming screen runs over the sample for the floor and then over
        // all rows; the sample is scored by the stream itself, so its floor carries the stream's bound
        p.form = PassForm::TwoStageStream;
        p.screen = stream_i8 ? Screen::GemvI8 : Screen::GemvBf16;
        p.fused_sample_seg = sample_segments(n_seg_all, n, a.topk, true, idx->sample_boost);
        p.dotf_rows = (int64_t)p.fused_sample_seg * orr::kSelSegRows;
        p.split_queries = !stream_i8;
        p.rowc_inline = stream_i8;
        p.approx_eps = stream_i8 ? kEpsI8 : eps_plain_bf16(D);
        p.eps1 = stream_i8 ? 0.0 : eps_plain_bf16(D);
        return ORR_OK;
    }
    // Where the two-stage pass applies it wins from the first MFMA batch on (1M x 3072 rows: 8 queries 2.19 ms against
    // 2.35 ms streaming, 32 queries 2.28 against 3.07, 64 queries 2.4 against 6.3)
    const bool two_stage = idx->opt_two_stage != 0 && floor_fits;
    if (B <= 64 && !two_stage) {        // HBM-bound streaming form over all rows, 32 queries per launch
        p.form = PassForm::StreamMfma;
        p.approx_eps = eps_f32_mfma(D);
        return ORR_OK;
    }
    // split bf16: queries split once; with enough rows the GEMM over everything behind a sampled prefix runs with the fused
    // scoring epilogue (once the floor keys exist) and only the prefix's dots go through HBM
    p.fused_sample_seg = ((idx->opt_fuse_epilogue || two_stage) && !a.no_fuse && n_seg_all >= 48)
                             ? sample_segments(n_seg_all, n, a.topk, false, idx->sample_boost) : 0;
    if (p.fused_sample_seg > 0) p.dotf_rows = (int64_t)p.fused_sample_seg * orr::kSelSegRows;
    p.split_queries = true;
    p.approx_eps = eps_split_bf16(D);
    if (!two_stage) {
        p.form = p.fused_sample_seg > 0 ? PassForm::SplitFused : PassForm::SplitAll;
        return ORR_OK;
    }
    // ---- two-stage: floor from the k-th best score of the prefix; ONE screening product over ALL rows keeps every row
    // that can still reach it; those are re-scored exactly; the best k' of them become the records.
    p.form = PassForm::TwoStageGemm;
    // Where the int8 shadow exists the prefix and the screen go through the int8 screening GEMM (integer dots out; the
    // per-pair bound turns them into LOWER bounds of the scores), which reads a quarter of the bytes of the split pass and
    // runs at twice its MFMA rate; else the screen runs on the bf16 shadow, else it converts the fp32 rows itself
    if (idx->opt_two_stage == 1 && D % 128 == 0) {
        ORR_TRY(ensure_i8_shadow(idx));
        p.prefix_i8 = idx->i8_ready;
    }
    if (idx->opt_two_stage == 1 && !p.prefix_i8) ORR_TRY(ensure_shadow(idx));
    p.screen = p.prefix_i8 ? Screen::I8Ranges : (idx->opt_two_stage == 1 && idx->shadow_ready) ? Screen::Bf16Shadow : Screen::Bf16x1;
    if (p.prefix_i8) {
        p.split_queries = false;
        p.approx_eps = kEpsI8;
    } else {
        p.eps1 = eps_plain_bf16(D);
    }
    // the prefix's floor: 0 its rows ranked in full; 1 per-lane maxima, sorted; 2 wave maxima, nothing sorted (where 16 per
    // segment are at least 8 k candidates per query)
    const char *prefix_env = getenv("ORR_PREFIX_FULL_RANKING");               // =1: form 0; =2: form 1 (A/B and the floor's tests: read at every plan)
    p.prefix_floor_form = (prefix_env && atoi(prefix_env) == 1) ? 0
                          : ((int64_t)p.fused_sample_seg * 16 >= 8 * (int64_t)std::max<int32_t>(1, a.topk) && !(prefix_env && atoi(prefix_env) == 2)) ? 2 : 1;
    // Large shards go through the int8 screening GEMM in FOUR ROW RANGES: only the first range's count words are formed
    // in front of the GEMM; those of the later ranges are formed on the keyword stream while the earlier ranges are
    // multiplied (the GEMM leaves half of the HBM bandwidth unused; in front of it the count words were 0.5 of the
    // 1.6 ms a 10M-row, 256-query batch spends before its GEMM starts, 2.7 of 6.9 ms at 12.5M rows x 1024 queries).
    const bool has_terms = qoff[(size_t)B] > qoff[0];
    if (has_terms && p.prefix_i8 && n >= (int64_t)2000000) {
        // four ranges, eight for more than 256 queries (the first range's count words sit in front of the GEMM: 4 planes
        // x 4 B per row and 32 queries)
        p.n_ranges = B > 256 ? 8 : 4;                     // (12.5M rows x 1024 queries: 43.0 / 41.1 / 41.0 ms per batch with 4 / 8 / 16)
        // (boundaries on whole rounds of the persistent GEMM -- 256 workgroups x 256-row tiles: every workgroup of a
        // launch then multiplies the same number of tiles; only the last range ends on a partial round)
        constexpr int64_t kRound = 256 * 256;
        for (int r = 1; r < p.n_ranges; ++r) p.range_row[r] = (n * r / p.n_ranges + kRound / 2) / kRound * kRound;
    }
    // two-bit count words where every query has at most three terms and the 16 x 16 x 64 form screens (its epilogue reads
    // them): half the words written and read
    uint32_t max_terms = 0;
    for (int32_t b = 0; b < B; ++b) max_terms = std::max(max_terms, qoff[(size_t)b + 1] - qoff[(size_t)b]);
    if (has_terms && max_terms <= 3 && p.prefix_i8 && orr::screen_i8_uses_tile16(B, n, D, (n + 63) / 64 * 64) && !getenv("ORR_COUNT_BITS4"))
        p.count_bits = 2;
    return ORR_OK;
}

// The plan of one pass: plan_form's, with what the escalation ladder takes for granted about it (orr_escalation.h).
int plan_pass(orr_index *idx, const BatchArgs &a, int32_t kprime, int64_t n, const std::vector<uint32_t> &qoff, PassPlan &p)
{
    ORR_TRY(plan_form(idx, a, kprime, n, qoff, p));
    // (host-resident batches were looked at: has_tiny_query.  The int8 forms carry a per-pair bound that is infinite for such a query.)
    p.keep_tiny = p.use_mfma && p.q_on_device && !p.prefix_i8 && p.screen != Screen::GemvI8;
    assert(!p.fused() || !a.no_fuse);
    assert(!p.use_mfma || !a.force_exact);
    assert(!p.two_stage() || p.fused());
    return ORR_OK;
}

// The shared scope of a masked search as its pass sees it (orr_search_batch_masked; the rules are orr_mask_plan.h's).
struct MaskScope {
    const uint32_t *bm = nullptr;       // device: the scope's bitmap over the shard's rows, deleted rows left out
    const uint32_t *chunks = nullptr;   // device: its chunk counts (launch_scope_counts)
    int64_t words = 0;
    int64_t live = 0, took = 0;         // live rows of the scope; the first `took` of them take part
    int64_t n_clip = 0;                 // one past the last of those: the pass runs over rows [0, n_clip)
    int64_t sample = 0;                 // rows of the in-scope sample the floor comes from (mask::sample_rows)
};

// The scopes of a grouped masked pass (orr_search_batch_masked_groups; the rules are orr_group_plan.h's): G bitmaps, each shared by
// the queries that name it.  The pass carries a MaskScope beside it (n_clip: the largest clip of a screen group, sample: the
// largest sample) for what the stages ask of a scope as a whole.
struct GroupScopes {
    int32_t n_groups = 0;
    const uint32_t *bm = nullptr;       // device [n_groups][words]: the groups' bitmaps, deleted rows left out
    const uint32_t *chunks = nullptr;   // device [n_groups][scope_chunks(words)]
    int64_t words = 0;
    std::vector<int64_t> took, n_clip, sample;   // per group: the rows that take part, one past the last of them, m_g
    const int64_t *d_clip = nullptr;    // device [n_groups]: n_clip of a screen group, 0 for the others
    const int64_t *d_sample = nullptr;  // device [n_groups]: m_g
    bool floor_heads = false;           // every query's sample fills 8 k lists (group::floor_from_heads)
    std::vector<int32_t> qgroup;        // the group of each query of the PASS (a sub-batch of the call)
    uint32_t cap = 0;                   // > 0: entries per query of the survivors' buffers of this pass (the call's own growth)
    // device, written by the floor stage of the pass: the group and the rows that took part per query
    const uint32_t *d_qgroup = nullptr;
    const int64_t *d_took = nullptr;
    uint32_t *h_screened = nullptr;     // pinned, a query per entry: under profiling the counts the screen left IN FRONT of the filter
};

// What the stages of one pass hand on to each other.
struct PassIo {
    const float *d_q = nullptr;         // the query vectors on the device
    double *d_dot = nullptr;            // exact dots [B][n]
    float *d_dotf = nullptr;            // approximate dots [B][dotf_rows]
    orr::KwView kw{nullptr, 0, nullptr, nullptr, nullptr};
    const double2 *d_rowc = nullptr;    // per-row selection constants, or null
    orr_candidate *d_cand = nullptr;    // the records [B][kprime + 1]
    bool direct_host = false;           // d_cand is pinned host memory
    const MaskScope *mask = nullptr;    // a masked pass: the scope (else null)
    GroupScopes *groups = nullptr;      // ... of several groups: their scopes (else null)
};

// The front end of a pass, unscoped (run_shard_once) or scoped (run_scoped_pass): the term offsets, the plan, where the
// records go, the query vectors where the kernels and the host finish read them.
struct PassFront {
    std::vector<uint32_t> qoff;         // query_term_off [B + 1], validated
    uint32_t n_terms_total = 0;
    size_t rec_bytes = 0;               // the records [B][kprime + 1]
    bool q_download_pending = false;    // device-resident vectors are on their way to the host (ev_q)
    PassIo io;
};

// Builds the front end: validates the term offsets, has the caller settle the plan (`plan(qoff, p)`, which reads them), places
// the records and stages the query vectors.  What differs between the callers: whether small record sets may go straight into
// pinned host memory (where the records carry their dots), whether BatchArgs::out_dev applies, whether the plan may leave the
// queries' exact norms to the device.  *q_host (if asked for): the vectors in host memory, valid until the next call.
template <class Plan>
int open_pass(orr_index *idx, const BatchArgs &a, int32_t kprime, Plan &&plan, bool pinned_records, bool out_dev, bool dev_norms,
              const float **q_host, PassPlan &p, PassFront &f)
{
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    if (q_host) *q_host = nullptr;
    f.qoff.resize((size_t)B + 1);
    memcpy(f.qoff.data(), a.query_term_off, sizeof(uint32_t) * ((size_t)B + 1));
    for (int32_t b = 0; b < B; ++b) {
        if (f.qoff[b + 1] < f.qoff[b]) return fail(ORR_EINVAL, "query_term_off is not monotone at query %d", b);
        if (f.qoff[b + 1] - f.qoff[b] > 65535) return fail(ORR_EINVAL, "query %d has more than 65535 terms", b);
    }
    f.n_terms_total = f.qoff[B] - f.qoff[0];
    if (f.n_terms_total > 0 && (!a.term_off || !a.terms_utf8)) return fail(ORR_EINVAL, "terms are referenced but term_off/terms_utf8 is NULL");

    ORR_TRY(plan(f.qoff, p));
    if (!dev_norms) p.dev_norms = false;
    idx->h_survivors.clear();

    // ---- record destination
    PassIo &io = f.io;
    f.rec_bytes = sizeof(orr_candidate) * (size_t)B * ((size_t)kprime + 1);
    io.direct_host = pinned_records && !p.use_mfma && f.rec_bytes <= (256u << 10);
    if (io.direct_host) {
        ORR_TRY(idx->pin_cand.reserve(f.rec_bytes));
        io.d_cand = idx->pin_cand.as<orr_candidate>();        // pinned host memory is device-writable
    } else if (out_dev && a.out_dev) {
        io.d_cand = a.out_dev;
    } else {
        ORR_TRY(idx->ws_cand.reserve(f.rec_bytes));
        io.d_cand = idx->ws_cand.as<orr_candidate>();
    }

    // ---- query vectors: the kernels read them where they are (device) or from one upload; device-resident ones get their
    // exact norms on the device (beside the first cosine kernel) or are downloaded for the host's pass
    idx->h_norm_a.assign((size_t)B, 0.0);
    if (!p.use_cos) return ORR_OK;
    const size_t qbytes = sizeof(float) * (size_t)B * a.dim;
    if (p.dev_norms) {
        io.d_q = a.q;
        ORR_TRY(idx->ws_norm_a.reserve(sizeof(double) * (size_t)B));
        ORR_TRY(idx->pin_norm.reserve(sizeof(double) * (size_t)B));
        HIP_TRY(orr::launch_dot_exact(io.d_q, B, a.dim, nullptr, 1, true, idx->ws_norm_a.as<double>(), B, idx->stream_aux));
        HIP_TRY(hipEventRecord(idx->ev_q, idx->stream_aux));
        return ORR_OK;
    }
    ORR_TRY(idx->pin_q.reserve(qbytes));
    if (p.q_on_device) {
        io.d_q = a.q;
        HIP_TRY(hipMemcpyAsync(idx->pin_q.p, a.q, qbytes, hipMemcpyDeviceToHost, idx->stream_kw));
        HIP_TRY(hipEventRecord(idx->ev_q, idx->stream_kw));
        f.q_download_pending = true;
    } else {
        memcpy(idx->pin_q.p, a.q, qbytes);
        ORR_TRY(idx->ws_q.reserve(qbytes));
        HIP_TRY(hipMemcpyAsync(idx->ws_q.p, idx->pin_q.p, qbytes, hipMemcpyHostToDevice, s));
        io.d_q = idx->ws_q.as<float>();
    }
    if (q_host) *q_host = idx->pin_q.as<float>();
    return ORR_OK;
}

// Records of a (sub-)batch no row takes part in: empty slots and, per query, the trailer of a pass that cut nothing.
std::vector<orr_candidate> empty_records(int32_t B, int32_t kprime)
{
    std::vector<orr_candidate> empty((size_t)B * ((size_t)kprime + 1));
    for (auto &c : empty) { memset(&c, 0, sizeof(c)); c.row_id = -1; c.order_key = -1; }
    for (int32_t b = 0; b < B; ++b) {
        orr_candidate &t = empty[(size_t)b * ((size_t)kprime + 1) + (size_t)kprime];
        t.approx_score = -std::numeric_limits<double>::infinity();
        t.order_key = 0; t.flags = ORR_CAND_TRAILER;
    }
    return empty;
}

// Large record sets (and those of a batched pass, whose dots are filled in last) reach pinned host memory in one copy.
int records_to_host(orr_index *idx, const PassFront &f, hipStream_t s)
{
    if (f.io.direct_host) return ORR_OK;
    ORR_TRY(idx->pin_cand.reserve(f.rec_bytes));
    HIP_TRY(hipMemcpyAsync(idx->pin_cand.p, f.io.d_cand, f.rec_bytes, hipMemcpyDeviceToHost, s));
    return ORR_OK;
}

// The int8 image of the queries.  The stream's (gemm = false) has one error term and its launch clears the pass's counters;
// the screening GEMM's has the second error term and is tiled like the rows.
int launch_i8_query_image(orr_index *idx, const float *d_q, int32_t B, bool gemm, hipStream_t s)
{
    ORR_TRY(idx->ws_q8.reserve(2 * (size_t)B * idx->dim));
    ORR_TRY(idx->ws_q8s1.reserve(sizeof(float) * (size_t)B));
    if (!gemm) {
        ORR_TRY(idx->ws_q8err.reserve(sizeof(double) * (size_t)B));
        ORR_TRY(idx->ws_fcnt.reserve(sizeof(uint32_t) * 3 * (size_t)B));
        HIP_TRY(orr::launch_i8_queries(d_q, B, idx->dim, idx->ws_q8.p, idx->ws_q8s1.as<float>(), idx->ws_q8err.as<double>(), s, nullptr,
                                       idx->ws_fcnt.as<uint32_t>(), 3 * B));
        return ORR_OK;
    }
    ORR_TRY(idx->ws_q8err.reserve(2 * sizeof(double) * (size_t)B));
    ORR_TRY(idx->ws_qtiled.reserve(orr::i8_tiled_bytes(B, idx->dim)));
    HIP_TRY(orr::launch_i8_queries(d_q, B, idx->dim, idx->ws_q8.p, idx->ws_q8s1.as<float>(), idx->ws_q8err.as<double>(), s,
                                   idx->ws_q8err.as<double>() + B));
    HIP_TRY(orr::launch_i8_tile_queries(idx->ws_q8.p, B, idx->dim, idx->ws_qtiled.p, s));
    return ORR_OK;
}

// Stage 5: the cosine numerators -- exact fp64 dots (Exact, LargeK), fp32 dots of all rows (StreamMfma, SplitAll) or of the
// sampled prefix (SplitFused, TwoStageGemm; the screening launch scores the rest).  The streaming form scores its prefix
// in the stream itself: it only needs the split queries (bf16) or the int8 image (made in stage 3).
int launch_numerators(orr_index *idx, const BatchArgs &a, const PassPlan &p, int64_t n, PassIo &io)
{
    if (!p.use_cos) return ORR_OK;
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    auto split_queries = [&]() -> int {
        ORR_TRY(idx->ws_qsplit.reserve(sizeof(float) * (size_t)B * idx->dim));
        HIP_TRY(orr::launch_split_queries(io.d_q, B, idx->dim, idx->ws_qsplit.p, s));
        return ORR_OK;
    };
    if (p.masked) {                     // no prefix under a mask (the floor comes from an in-scope sample): only the images the screen reads
        if (p.prefix_i8) return launch_i8_query_image(idx, io.d_q, B, true, s);
        return p.split_queries ? split_queries() : ORR_OK;
    }
    switch (p.form) {
    case PassForm::Exact:
    case PassForm::LargeK:
        ORR_TRY(idx->ws_dot.reserve(sizeof(double) * (size_t)B * (size_t)n));
        io.d_dot = idx->ws_dot.as<double>();
        for (int32_t b0 = 0; b0 < B; b0 += orr::kMaxExactQ) {
            const int32_t nq = std::min<int32_t>(orr::kMaxExactQ, B - b0);
            Timed t(idx, "dot_exact", 4.0 * (double)n * idx->dim + 4.0 * nq * idx->dim + 8.0 * nq * (double)n);
            HIP_TRY(orr::launch_dot_exact(idx->d_emb, n, idx->dim, io.d_q + (size_t)b0 * a.dim, nq, false,
                                          io.d_dot + (size_t)b0 * n, n, s));
        }
        return ORR_OK;
    case PassForm::TwoStageStream:
        if (p.split_queries) ORR_TRY(split_queries());
        return ORR_OK;
    case PassForm::StreamMfma:
        ORR_TRY(idx->ws_dotf.reserve(sizeof(float) * (size_t)B * (size_t)n));
        io.d_dotf = idx->ws_dotf.as<float>();
        for (int32_t b0 = 0; b0 < B; b0 += 32) {
            const int32_t nq = std::min<int32_t>(32, B - b0);
            Timed t(idx, "gemv_mfma", 4.0 * (double)n * idx->dim + 4.0 * (double)nq * idx->dim + 4.0 * (double)nq * (double)n);
            HIP_TRY(orr::launch_gemv_mfma(io.d_q + (size_t)b0 * a.dim, nq, idx->d_emb, n, idx->dim, io.d_dotf + (size_t)b0 * n, n, s));
        }
        return ORR_OK;
    default:                            // SplitAll, SplitFused, TwoStageGemm
        break;
    }
    const int64_t dotf_rows = p.dotf_rows;
    ORR_TRY(idx->ws_dotf.reserve(sizeof(float) * (size_t)B * (size_t)dotf_rows));
    io.d_dotf = idx->ws_dotf.as<float>();
    if (p.prefix_i8) {
        ORR_TRY(launch_i8_query_image(idx, io.d_q, B, true, s));
        const int64_t pre_rows = std::min<int64_t>(dotf_rows, n);
        Timed t(idx, "screen_i8_prefix", 1.0 * (double)pre_rows * idx->dim + 1.0 * (double)B * idx->dim + 4.0 * (double)B * (double)pre_rows);
        HIP_TRY(orr::launch_screen_i8_dots(idx->ws_qtiled.p, B, idx->emb_i8.p, pre_rows, idx->dim, io.d_dotf, dotf_rows, s));
    } else {
        ORR_TRY(split_queries());
        Timed t(idx, "gemm_dot_bf16x3", 4.0 * (double)dotf_rows * idx->dim + 4.0 * (double)B * idx->dim + 4.0 * (double)B * (double)dotf_rows);
        HIP_TRY(orr::launch_gemm_dot_bf16x3(idx->ws_qsplit.p, B, idx->d_emb, 0, dotf_rows, idx->dim, io.d_dotf, dotf_rows, nullptr, 3, s));
    }
    return ORR_OK;
}

// Stage 6: per-query constants (exact normA needs the vectors on the host, or comes from the device) and the per-row
// selection constants, which do not depend on the keyword side: enqueued before the main stream waits for it.
int launch_consts(orr_index *idx, const BatchArgs &a, const PassPlan &p, int64_t n, const std::vector<uint32_t> &qoff,
                  bool download_pending, PassIo &io)
{
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    if (download_pending) HIP_TRY(hipEventSynchronize(idx->ev_q));
    ORR_TRY(idx->pin_qc.reserve(sizeof(orr::QueryConst) * (size_t)B));
    ORR_TRY(idx->ws_qc.reserve(sizeof(orr::QueryConst) * (size_t)B));
    orr::QueryConst *qc = idx->pin_qc.as<orr::QueryConst>();
    const double tiny_below = p.keep_tiny ? (double)idx->dim * 0x1p-96 : 0.0;      // (max|q| < 2^-48 implies norm_a < D 2^-96)
    if (p.use_cos && !p.dev_norms) {
        if (a.norms_host) memcpy(idx->h_norm_a.data(), a.norms_host, sizeof(double) * (size_t)B);
        else exact_norms(idx->pin_q.as<float>(), B, a.dim, idx->h_norm_a.data());
    }
    for (int32_t b = 0; b < B; ++b) {
        qc[b].use_cos = p.use_cos ? 1 : 0;
        qc[b].norm_a = idx->h_norm_a[(size_t)b];
        qc[b].n_terms = (int32_t)(qoff[b + 1] - qoff[b]);
        qc[b].inv_n_terms = qc[b].n_terms > 0 ? 1.0 / (double)qc[b].n_terms : 0.0;
        qc[b].inv_sqrt_na = 0.0;
        if (p.batched_score && p.use_cos && !p.dev_norms) {
            if (qc[b].norm_a <= 0.0) qc[b].use_cos = 0;                    // guard :84 -> cosine 0 for every row
            else qc[b].inv_sqrt_na = 1.0 / std::sqrt(qc[b].norm_a);        // NaN stays NaN
            if (qc[b].norm_a > 0.0 && qc[b].norm_a < tiny_below) qc[b].use_cos |= orr::kQueryKeepAll;
        }
    }
    if (p.dev_norms) {        // (the kernel that adds the norms reads the host's constants in place: no upload command)
        HIP_TRY(hipStreamWaitEvent(s, idx->ev_q, 0));
        HIP_TRY(orr::launch_patch_query_norms(idx->ws_qc.as<orr::QueryConst>(), idx->ws_norm_a.as<double>(), B, p.batched_score, s,
                                              idx->pin_norm.as<double>(), qc, tiny_below));
    } else {
        HIP_TRY(hipMemcpyAsync(idx->ws_qc.p, qc, sizeof(orr::QueryConst) * (size_t)B, hipMemcpyHostToDevice, s));
    }
    if (p.batched_score && !p.rowc_inline) {
        ORR_TRY(idx->ws_rowc.reserve(sizeof(double2) * (size_t)n));
        Timed t(idx, io.groups ? "row_consts_grouped" : io.mask ? "row_consts_masked" : "row_consts", 32.0 * (double)n);
        if (io.groups)    // rows outside every screen group's clipped scope get constants below every floor
            HIP_TRY(orr::launch_row_consts_grouped(idx->d_norm_b, idx->d_created, a.now_ticks, n, io.groups->bm, io.groups->words,
                                                   io.groups->n_groups, io.groups->d_clip, idx->ws_rowc.as<double2>(), s));
        else if (io.mask) // rows outside the scope get constants below every floor
            HIP_TRY(orr::launch_row_consts_masked(idx->d_norm_b, idx->d_created, a.now_ticks, n, io.mask->bm, idx->ws_rowc.as<double2>(), s));
        else
            HIP_TRY(orr::launch_row_consts(idx->d_norm_b, idx->d_created, a.now_ticks, n, idx->ws_rowc.as<double2>(), s));
        io.d_rowc = idx->ws_rowc.as<double2>();
    }
    return ORR_OK;
}

// The kernel that re-scores buffered survivors in the reference arithmetic, and with it whether anybody reads their counts.
enum class Rescore {
    BufferExact,    // rescore_buffer_exact (a cosine part, dim % 64 == 0), inside finish_survivors where dim % 256 == 0; the
                    // survivors' counts go back with the records (idx->pin_cnt)
    ScopeGeneric,   // scope_rescore: any dimension, queries without a cosine part (a scoped pass); the host knows the counts
};

// Exact re-score of every buffered survivor into idx->ws_fdot, as its own launch.
int rescore_survivors(orr_index *idx, const BatchArgs &a, const PassIo &io, const orr::FusedEpilogue &epi, uint32_t kCap, Rescore how,
                      double bytes, hipStream_t s)
{
    Timed t(idx, how == Rescore::BufferExact ? "rescore_buffer_exact" : "scope_rescore", bytes);
    HIP_TRY((how == Rescore::BufferExact ? orr::launch_rescore_buffer_exact : orr::launch_scope_rescore_generic)(
        idx->d_emb, idx->dim, io.d_q, a.B, idx->d_norm_b, idx->d_created, io.kw, idx->ws_qc.as<orr::QueryConst>(), a.now_ticks, epi.cnt, kCap,
        epi.buf, idx->ws_fdot.as<double>(), s));
    return ORR_OK;
}

// The tail of the two-stage pass and of a scoped Selection pass: exact re-score of every buffered survivor (fp32 master,
// reference arithmetic), the best k' of them as records with their exact dots.  BufferExact and dim % 256 == 0:
// finish_survivors (four lanes per survivor, or a wave per survivor for the smallest batches; the workgroup that draws a
// query's last ticket -- or a second launch -- merges its lists and writes the records, straight into pinned host memory when
// the record set is small); else four launches, the first of them `how` (Timed bytes: rescore_bytes).
int two_stage_tail(orr_index *idx, const BatchArgs &a, int32_t kprime, int64_t n, PassIo &io, const orr::FusedEpilogue &epi,
                   uint32_t kCap, int32_t buf_lists, bool host_records, size_t rec_bytes, Rescore how, double rescore_bytes, hipStream_t s)
{
    const int32_t B = a.B;
    ORR_TRY(idx->ws_fdot.reserve(sizeof(double) * (size_t)B * kCap));
    ORR_TRY(idx->pin_cnt.reserve(sizeof(uint32_t) * (size_t)B));
    if (how == Rescore::BufferExact && B <= kFinishFusedMaxB && idx->dim % 256 == 0) {
        // the tail in one launch; small record sets go straight into pinned host memory (they are final when written)
        if (host_records && !a.out_dev && rec_bytes <= (256u << 10)) {
            ORR_TRY(idx->pin_cand.reserve(rec_bytes));
            io.d_cand = idx->pin_cand.as<orr_candidate>();
            io.direct_host = true;
        }
        Timed t(idx, "finish_survivors", 0.0);
        HIP_TRY(orr::launch_finish_survivors(idx->d_emb, idx->dim, io.d_q, B, idx->d_norm_b, idx->d_created, idx->d_row_ids, io.kw,
                                             idx->ws_qc.as<orr::QueryConst>(), a.now_ticks, epi.cnt, idx->ws_fcnt.as<uint32_t>() + 2 * B,
                                             kCap, epi.buf, idx->ws_fdot.as<double>(), idx->ws_sel.as<orr::SelEntry>(), kprime, n,
                                             idx->row_base, idx->ws_tsL.as<double>(), io.d_cand, idx->pin_cnt.as<uint32_t>(), s));
    } else {
        ORR_TRY(rescore_survivors(idx, a, io, epi, kCap, how, rescore_bytes, s));
        {
            Timed t(idx, "buffer_to_lists", 0.0);
            HIP_TRY(orr::launch_buffer_to_lists(epi.buf, epi.cnt, kCap, B, 0, buf_lists, idx->ws_sel.as<orr::SelEntry>(), s));
        }
        {
            Timed t(idx, "select_final", (double)B * (double)buf_lists * orr::kSelWidth * sizeof(orr::SelEntry));
            HIP_TRY(orr::launch_select_final(idx->ws_sel.as<orr::SelEntry>(), buf_lists, B, kprime, n, idx->row_base,
                                             nullptr, nullptr, 0, idx->d_norm_b, idx->d_created, idx->d_row_ids, io.kw,
                                             0, 0.0, nullptr, epi.cnt, kCap, idx->ws_tsL.as<double>(), io.d_cand, s));
        }
        {   // the records' exact dots come out of the buffer: no second K6 pass
            Timed t(idx, "records_dot_from_buffer", 0.0);
            HIP_TRY(orr::launch_records_dot_from_buffer(epi.buf, idx->ws_fdot.as<double>(), epi.cnt, kCap, B, kprime, idx->row_base,
                                                        io.d_cand, s));
        }
        // the survivors' counts go back with the records: per-query escalation and orr_index_search_stats
        if (how == Rescore::BufferExact)
            HIP_TRY(hipMemcpyAsync(idx->pin_cnt.p, epi.cnt, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
    }
    return ORR_OK;
}

// The int8 screening GEMM (K2j) with the fused scoring epilogue over all participating rows, in p.n_ranges row ranges: the
// later ranges' count words are formed on the keyword stream while the earlier ranges are multiplied (released when the main
// stream gets here), every launch draws its output tiles from its own set of tickets (cleared by fused_query_consts).
int screen_i8_in_ranges(orr_index *idx, const BatchArgs &a, const PassPlan &p, int64_t n, const orr::KwView &kw,
                        orr::FusedEpilogue epi, hipStream_t s)
{
    const int32_t B = a.B;
    const int64_t *range_row = p.range_row;
    // algorithmic bytes: the int8 rows once, per row its constants (rowc 16 B, i8_rowf 16 B) and, with query terms,
    // 16 B of count words per 32 queries; the query image once
    if (p.n_ranges > 1) {
        // the later ranges' count words: released when the main stream reaches the first range's GEMM
        hipStream_t k = idx->stream_kw;
        HIP_TRY(hipEventRecord(idx->ev_main_ready, s));
        HIP_TRY(hipStreamWaitEvent(k, idx->ev_main_ready, 0));
        for (int r = 1; r < p.n_ranges; ++r) {
            {
                Timed t(idx, "count_planes", p.plane_bytes_per_row(B) * (double)(range_row[r + 1] - range_row[r]), k);
                HIP_TRY(orr::launch_query_count_planes(kw, B, n, epi.plane_stride, idx->ws_fany.as<uint32_t>(), k, range_row[r],
                                                       range_row[r + 1], epi.count_bits == 2 ? 2 : 4));
            }
            HIP_TRY(hipEventRecord(idx->ev_range[r - 1], k));
        }
    }
    for (int r = 0; r < p.n_ranges; ++r) {
        if (r > 0) HIP_TRY(hipStreamWaitEvent(s, idx->ev_range[r - 1], 0));
        epi.tickets = idx->ws_tickets.as<uint32_t>() + 8 * r;
        const double rows_r = (double)(range_row[r + 1] - range_row[r]);
        Timed t(idx, "screen_i8_fused", rows_r * ((double)idx->dim + 32.0 + (epi.count_planes ? (epi.count_bits == 2 ? 8.0 : 16.0) * (double)((B + 31) / 32) : 0.0)) +
                                        1.0 * (double)B * idx->dim);
        HIP_TRY(orr::launch_screen_i8(idx->ws_qtiled.p, B, idx->emb_i8.p, range_row[r + 1], idx->dim, epi, s, range_row[r]));
    }
    return ORR_OK;
}

// The floor of a masked pass: the first mask.sample in-scope rows become buffer entries, the exact re-score gives them exact
// keys, and their kth best per query is the floor's base -- a lower bound of the final kth best whatever the scope looks like.
// The keys are exact scores of the device's arithmetic: the floor carries the certificate's own bound, no screen's.
// orr_index_capture_screen: the handle whose capture a pass on this lane records into (an internal lane: its owner's).
orr_index *capture_handle(orr_index *lane) { return lane->internal_lane && lane->parent ? const_cast<orr_index *>(lane->parent) : lane; }

// The capture point of screen_two_stage: behind the screen and the scope filter, in front of the exact tail.  Waits for the
// stream, copies the floor, the counters and the buffers of all B queries to the handle and disarms it; launches nothing.
int capture_screen(orr_index *idx, const BatchArgs &a, const PassPlan &p, int64_t n, const PassIo &io, const orr::FloorOut &floor,
                   const orr::FusedEpilogue &epi, uint32_t kCap, int32_t kth, hipStream_t s)
{
    ScreenCapture &c = capture_handle(idx)->capture;
    const size_t B = (size_t)a.B;
    c.armed.store(0, std::memory_order_relaxed);            // one capture per arming, whether or not this one succeeds
    c.have = false;
    c.floor_key.resize(B); c.L.resize(B); c.cnt.resize(B); c.buf.resize(B * (size_t)kCap);
    HIP_TRY(hipMemcpyAsync(c.floor_key.data(), floor.floor_key, sizeof(unsigned long long) * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c.L.data(), floor.L, sizeof(double) * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c.cnt.data(), epi.cnt, sizeof(uint32_t) * B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c.buf.data(), epi.buf, sizeof(orr::SelEntry) * B * (size_t)kCap, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    orr_screen_capture &o = c.info;
    o = orr_screen_capture{};
    o.B = a.B; o.kth = kth; o.cap = kCap;
    o.screen = (int32_t)p.screen;
    o.tile_form = p.screen == Screen::I8Ranges ? orr::screen_i8_form(a.B, p.range_row[1], idx->dim, epi) : -1;
    o.scope = io.groups ? 2 : io.mask ? 1 : 0;
    o.floor_form = io.mask || p.stream() ? -1 : p.prefix_floor_form;
    o.n = n;
    o.prefix_rows = io.mask ? io.mask->sample : std::min<int64_t>(p.dotf_rows, n);
    o.eps3 = floor.eps3; o.eps1 = floor.eps1;
    c.have = true;
    return ORR_OK;
}

// (floor.eps3 becomes the bound the sample's exact keys carry: what the floor's launch gets, and what a capture reports)
int masked_floor(orr_index *idx, const BatchArgs &a, const PassIo &io, int32_t kth, orr::FloorOut &floor)
{
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    const MaskScope &m = *io.mask;
    GroupScopes *gs = io.groups;
    const uint32_t cap = (uint32_t)m.sample;                                   // whole lists of 64, fewer than took
    const int32_t lists = (int32_t)(cap / orr::kSelWidth);
    // [limit i64][query -> bitmap 0, u32 x B][counts u32 x B]; grouped: [rows that took part, i64 x B][query -> its group's
    // bitmap][counts: its group's sample <= cap], the limits per bitmap are the call's (GroupScopes::d_sample)
    const size_t o_sel = sizeof(int64_t) * (gs ? (size_t)B : 1), o_cnt = o_sel + sizeof(uint32_t) * (size_t)B, bytes = o_cnt + sizeof(uint32_t) * (size_t)B;
    ORR_TRY(idx->pin_mask.reserve(sizeof(int64_t) + bytes));                   // (its first word: n_clip, masked_batch's)
    ORR_TRY(idx->ws_mask_cnt.reserve(bytes));
    uint8_t *hp = idx->pin_mask.as<uint8_t>() + sizeof(int64_t);
    if (!gs) *reinterpret_cast<int64_t *>(hp) = m.sample;
    for (int32_t b = 0; b < B; ++b) {
        const int32_t g = gs ? gs->qgroup[(size_t)b] : 0;
        if (gs) reinterpret_cast<int64_t *>(hp)[b] = gs->took[(size_t)g];
        reinterpret_cast<uint32_t *>(hp + o_sel)[b] = (uint32_t)g;
        reinterpret_cast<uint32_t *>(hp + o_cnt)[b] = gs ? (uint32_t)gs->sample[(size_t)g] : cap;
    }
    HIP_TRY(hipMemcpyAsync(idx->ws_mask_cnt.p, hp, bytes, hipMemcpyHostToDevice, s));
    uint8_t *dp = idx->ws_mask_cnt.as<uint8_t>();
    const uint32_t *d_cnt = reinterpret_cast<const uint32_t *>(dp + o_cnt);
    if (gs) { gs->d_took = reinterpret_cast<const int64_t *>(dp); gs->d_qgroup = reinterpret_cast<const uint32_t *>(dp + o_sel); }
    ORR_TRY(idx->ws_pbuf.reserve(sizeof(orr::SelEntry) * (size_t)B * cap));
    ORR_TRY(idx->ws_psel.reserve(sizeof(orr::SelEntry) * (size_t)B * cap));
    ORR_TRY(idx->ws_dot.reserve(sizeof(double) * (size_t)B * cap));
    orr::SelEntry *buf = idx->ws_pbuf.as<orr::SelEntry>();
    {
        Timed t(idx, "mask_sample_compact", 16.0 * (double)B * (double)cap);
        if (gs)
            HIP_TRY(orr::launch_scope_compact(gs->bm, gs->words, gs->n_groups, gs->chunks, gs->d_qgroup, B, gs->d_sample, buf, cap, s));
        else
            HIP_TRY(orr::launch_scope_compact(m.bm, m.words, 1, m.chunks, reinterpret_cast<const uint32_t *>(dp + o_sel), B,
                                              reinterpret_cast<const int64_t *>(dp), buf, cap, s));
    }
    {
        Timed t(idx, "mask_sample_rescore", (double)B * (double)cap * 4.0 * idx->dim);
        HIP_TRY(orr::launch_rescore_buffer_exact(idx->d_emb, idx->dim, io.d_q, B, idx->d_norm_b, idx->d_created, io.kw,
                                                 idx->ws_qc.as<orr::QueryConst>(), a.now_ticks, d_cnt, cap, buf, idx->ws_dot.as<double>(), s));
    }
    Timed t(idx, "mask_sample_floor", 0.0);
    HIP_TRY(orr::launch_buffer_to_lists(buf, d_cnt, cap, B, 0, lists, idx->ws_psel.as<orr::SelEntry>(), s));
    floor.eps3 = kCertifyEps;
    // (grouped: the lists behind a query's own sample are empty, so the heads alone serve only where every sample fills 8 k lists)
    HIP_TRY(orr::launch_select_final_sample(idx->ws_psel.as<orr::SelEntry>(), lists, lists, B, kth, idx->ws_tau.as<unsigned long long>(), s, floor,
                                            0, gs && !gs->floor_heads ? 1 : 0));
    return ORR_OK;
}

// The two-stage forms after the prefix: the floor, the screen over all rows into the survivors' buffers, the exact tail.
int screen_two_stage(orr_index *idx, const BatchArgs &a, const PassPlan &p, int32_t kprime, int64_t n, PassIo &io,
                     orr::FusedEpilogue &epi, uint32_t kCap, int32_t buf_lists, int32_t lists_total, bool host_records, size_t rec_bytes)
{
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    const int32_t kth = std::max<int32_t>(1, a.topk);
    unsigned long long *d_tau = idx->ws_tau.as<unsigned long long>();
    ORR_TRY(idx->ws_tsL.reserve(sizeof(double) * (size_t)B));
    ORR_TRY(idx->ws_tskey.reserve(sizeof(unsigned long long) * (size_t)B));
    // the floor comes out of the sampling selection's own launch
    orr::FloorOut floor;
    floor.floor_key = idx->ws_tskey.as<unsigned long long>();
    floor.L = idx->ws_tsL.as<double>();
    floor.eps3 = p.approx_eps; floor.eps1 = p.eps1;
    if (io.mask) ORR_TRY(masked_floor(idx, a, io, kth, floor));
    if (io.mask && p.stream()) {
        // (the stream scores in fp64 against the floor keys directly: nothing more in front of it)
    } else if (p.stream()) {
        // the sample goes through the stream too: floor keys of 0 keep every sampled row, their
        // approximate keys are sorted in lists of 64 and the k-th best one per query is the floor's base
        const uint32_t cap_p = (uint32_t)p.dotf_rows;                 // a multiple of 4096
        ORR_TRY(idx->ws_pbuf.reserve(sizeof(orr::SelEntry) * (size_t)B * cap_p));
        if (idx->ws_zero.cap < sizeof(unsigned long long) * (size_t)B) {   // floor keys of 0, never written again
            ORR_TRY(idx->ws_zero.reserve(sizeof(unsigned long long) * (size_t)std::max<int32_t>(B, 64)));
            HIP_TRY(hipMemsetAsync(idx->ws_zero.p, 0, idx->ws_zero.cap, s));
        }
        const bool i8 = p.screen == Screen::GemvI8;
        orr::FusedEpilogue pre = epi;
        pre.tau = idx->ws_zero.as<unsigned long long>();
        pre.buf = idx->ws_pbuf.as<orr::SelEntry>();
        pre.cap = cap_p;
        pre.cnt = idx->ws_fcnt.as<uint32_t>() + B;         // its own counters: one clearing for both launches
        const int64_t pre_rows = std::min<int64_t>(p.dotf_rows, n);
        const bool pre_lists = i8 && orr::screen_gemv_i8_prefix_makes_lists(idx->dim);   // sorted lists straight from the kernel
        ORR_TRY(idx->ws_psel.reserve(sizeof(orr::SelEntry) * (size_t)B * cap_p));
        if (pre_lists) pre.buf = idx->ws_psel.as<orr::SelEntry>();
        {
            Timed t(idx, "screen_gemv_prefix", (i8 ? 1.0 : 2.0) * (double)p.dotf_rows * idx->dim + 2.0 * (double)B * idx->dim);
            if (i8)
                HIP_TRY(orr::launch_screen_gemv_i8(idx->ws_q8.p, idx->ws_q8s1.as<float>(), idx->ws_q8err.as<double>(), B, idx->emb_i8.p,
                                                   idx->i8_scale.as<float>(), idx->i8_rel_err.as<float>(), idx->i8_rel_hat.as<float>(),
                                                   idx->d_norm_b, idx->d_created, a.now_ticks, pre_rows, idx->dim, pre, true, s));
            else
                HIP_TRY(orr::launch_screen_gemv_bf16(idx->ws_qsplit.p, B, idx->emb_shadow.p, pre_rows, idx->dim, pre, s));
        }
        {   // lists of 64 sorted in parallel (by the int8 stream itself where it can), then the k-th best key per query
            Timed t(idx, "select_floor", 0.0);
            const int32_t lists_all = (int32_t)(cap_p / orr::kSelWidth);
            const int32_t lists_p = pre_lists ? (int32_t)((pre_rows + orr::kSelWidth - 1) / orr::kSelWidth) : lists_all;
            if (!pre_lists)
                HIP_TRY(orr::launch_buffer_to_lists(pre.buf, pre.cnt, cap_p, B, 0, lists_all, idx->ws_psel.as<orr::SelEntry>(), s));
            HIP_TRY(orr::launch_select_final_sample(idx->ws_psel.as<orr::SelEntry>(), lists_all, lists_p, B, kth, d_tau, s, floor));
        }
    } else {
        if (!io.mask) {
            Timed t(idx, "select_floor", 0.0);
            HIP_TRY(orr::launch_select_final_sample(idx->ws_sel.as<orr::SelEntry>(), lists_total, p.fused_sample_seg, B, kth, d_tau, s, floor,
                                                    p.prefix_floor_form == 2 ? 1 : 0));
        }
        const bool gemm_i8 = p.screen == Screen::I8Ranges;
        if (gemm_i8) {
            epi.i8_rowf = idx->i8_rowf.as<float4>();
            epi.i8_qs1 = idx->ws_q8s1.as<float>();
        }
        // (ws_fqf holds two arrays of B: qf, and behind it the NaN-safe copy the 16 x 16 x 64 form stages; the streaming
        // kernels score in fp64 directly, no fp32 pre-filter constants)
        HIP_TRY(orr::launch_fused_query_consts(idx->ws_qc.as<orr::QueryConst>(), idx->ws_tskey.as<unsigned long long>(), B,
                                               idx->ws_fqf.as<float4>(), s, gemm_i8 ? idx->ws_q8s1.as<float>() : nullptr,
                                               gemm_i8 ? idx->ws_q8err.as<double>() + B : nullptr,
                                               gemm_i8 ? idx->ws_fqf.as<float4>() + B : nullptr,
                                               idx->ws_fcnt.as<uint32_t>(), 3 * B, idx->ws_tickets.as<uint32_t>(), 8 * 16));
        epi.qf16 = gemm_i8 ? idx->ws_fqf.as<float4>() + B : nullptr;
    }
    epi.tau = idx->ws_tskey.as<unsigned long long>();
    if (p.screen == Screen::I8Ranges) {
        ORR_TRY(screen_i8_in_ranges(idx, a, p, n, io.kw, epi, s));
    } else if (p.screen == Screen::GemvI8) {
        Timed t(idx, "screen_gemv_i8", 1.0 * (double)n * idx->dim + 28.0 * (double)n + 2.0 * (double)B * idx->dim);   // per row: scale, two relative norms (12 B), normB and created (16 B)
        HIP_TRY(orr::launch_screen_gemv_i8(idx->ws_q8.p, idx->ws_q8s1.as<float>(), idx->ws_q8err.as<double>(), B, idx->emb_i8.p,
                                           idx->i8_scale.as<float>(), idx->i8_rel_err.as<float>(), idx->i8_rel_hat.as<float>(),
                                           io.mask ? nullptr : idx->d_norm_b, idx->d_created, a.now_ticks, n, idx->dim, epi, false, s));   // (masked: the constants come from epi.rowc)
    } else if (p.screen == Screen::GemvBf16) {
        Timed t(idx, "screen_gemv_bf16", 2.0 * (double)n * idx->dim + 2.0 * (double)B * idx->dim);
        HIP_TRY(orr::launch_screen_gemv_bf16(idx->ws_qsplit.p, B, idx->emb_shadow.p, n, idx->dim, epi, s));
    } else if (p.screen == Screen::Bf16Shadow) {
        ORR_TRY(idx->ws_qtiled.reserve(orr::bf16_tiled_bytes(B, idx->dim)));
        HIP_TRY(orr::launch_bf16_tiled(io.d_q, B, idx->dim, idx->ws_qtiled.p, s));
        Timed t(idx, "screen_bf16_fused", 2.0 * (double)n * idx->dim + 2.0 * (double)B * idx->dim);
        HIP_TRY(orr::launch_screen_bf16(idx->ws_qtiled.p, B, idx->emb_shadow.p, 0, n, idx->dim, nullptr, 0, &epi, s));
    } else {
        Timed t(idx, "gemm_dot_bf16x1_fused", 4.0 * (double)n * idx->dim + 2.0 * (double)B * idx->dim);
        HIP_TRY(orr::launch_gemm_dot_bf16x3(idx->ws_qsplit.p, B, idx->d_emb, 0, n, idx->dim, nullptr, 0, &epi, 1, s));
    }
    if (io.groups) {    // ... of the query's own group: a row of another group that beat the query's floor goes here
        if (idx->profiling == 1 && io.groups->h_screened)      // (kernel statistics: what the screen buffered, other groups' rows included)
            HIP_TRY(hipMemcpyAsync(io.groups->h_screened, epi.cnt, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost, s));
        Timed t(idx, "mask_survivors_grouped", 16.0 * (double)B * (double)kCap);
        HIP_TRY(orr::launch_mask_survivors_grouped(io.groups->bm, io.groups->words, io.groups->n_groups, io.groups->d_clip, io.groups->d_qgroup,
                                                   epi.cnt, kCap, epi.buf, B, s));
    } else if (io.mask) {      // the one exact application of the mask: what the screen buffered from outside the scope goes
        Timed t(idx, "mask_survivors", 16.0 * (double)B * (double)kCap);
        HIP_TRY(orr::launch_mask_survivors(io.mask->bm, io.mask->n_clip, epi.cnt, kCap, epi.buf, B, s));
    }
    if (capture_handle(idx)->capture.armed.load(std::memory_order_relaxed)) ORR_TRY(capture_screen(idx, a, p, n, io, floor, epi, kCap, kth, s));
    ORR_TRY(two_stage_tail(idx, a, kprime, n, io, epi, kCap, buf_lists, host_records, rec_bytes, Rescore::BufferExact, 0.0, s));
    if (io.groups) HIP_TRY(orr::launch_mask_trailers_grouped(io.d_cand, B, kprime, io.groups->d_took, s));
    else if (io.mask) HIP_TRY(orr::launch_mask_trailers(io.d_cand, B, kprime, io.mask->took, s));
    return ORR_OK;
}

// Stage 7 of the SplitFused and two-stage forms: prefix lists -> floor keys -> the screening launch with the scoring
// epilogue -> survivors' buffers -> lists (SplitFused: the final merge reads prefix lists + buffer lists) or the exact tail.
int select_fused(orr_index *idx, const BatchArgs &a, const PassPlan &p, int32_t kprime, int64_t n, PassIo &io, bool host_records,
                 size_t rec_bytes)
{
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    uint32_t kCap = idx->survivor_cap;                              // survivors kept per query (a multiple of 64)
    if (io.groups && io.groups->cap) kCap = io.groups->cap;         // (a grouped call's own growth: the lane does not keep it)
    while (kCap > 8192 && (size_t)B * kCap * 40 > ((size_t)2 << 30)) kCap >>= 1;
    idx->pass_cap = kCap;
    const int32_t fss = p.fused_sample_seg;
    const int32_t buf_lists = (int32_t)(kCap / orr::kSelWidth);
    const int32_t lists_total = fss + buf_lists;
    const int32_t finish_group = orr::finish_survivors_group(B, idx->dim);      // (finish_survivors' lists: one per group)
    const int32_t lists_room = std::max<int32_t>(lists_total, finish_group ? (int32_t)(kCap / (uint32_t)finish_group) : 0);
    ORR_TRY(idx->ws_sel.reserve(sizeof(orr::SelEntry) * (size_t)B * (size_t)lists_room * orr::kSelWidth));
    ORR_TRY(idx->ws_tau.reserve(sizeof(unsigned long long) * (size_t)B));
    ORR_TRY(idx->ws_fcnt.reserve(sizeof(uint32_t) * 3 * (size_t)B));      // [survivors][sampled prefix][workgroups done]
    ORR_TRY(idx->ws_fbuf.reserve(sizeof(orr::SelEntry) * (size_t)B * kCap));
    unsigned long long *d_tau = idx->ws_tau.as<unsigned long long>();
    if (!p.stream() && !io.mask) {
        Timed t(idx, "fuse_select", (double)B * (double)p.dotf_rows * 28.0);
        orr::I8Prefix i8p;
        if (p.prefix_i8) { i8p.rowf = idx->i8_rowf.as<float4>(); i8p.qs1 = idx->ws_q8s1.as<float>(); i8p.qerr2 = idx->ws_q8err.as<double>() + B; }
        HIP_TRY(orr::launch_fuse_select(nullptr, io.d_dotf, p.dotf_rows, idx->d_norm_b, idx->d_created, io.d_rowc, io.kw,
                                        idx->ws_qc.as<orr::QueryConst>(), a.now_ticks, std::min<int64_t>(p.dotf_rows, n), B, 0, fss,
                                        nullptr, idx->ws_sel.as<orr::SelEntry>(), lists_total, s, i8p,
                                        // two-stage: the prefix only yields the floor (the records come out of the survivors' buffers)
                                        p.prefix_floor_form));
    }
    ORR_TRY(idx->ws_fqf.reserve(sizeof(float4) * 2 * (size_t)B));
    orr::FusedEpilogue epi{};
    epi.plane_stride = (n + 63) / 64 * 64;
    if (io.kw.bitmaps && !p.stream()) {
        ORR_TRY(idx->ws_fany.reserve(sizeof(uint32_t) * orr::kCountPlanes * (size_t)((B + 31) / 32) * (size_t)epi.plane_stride));
        epi.count_bits = p.count_bits;
        Timed t(idx, "count_planes", p.plane_bytes_per_row(B) * (double)(p.range_row[1] - p.range_row[0]));
        HIP_TRY(orr::launch_query_count_planes(io.kw, B, n, epi.plane_stride, idx->ws_fany.as<uint32_t>(), s, 0, p.range_row[1],
                                               epi.count_bits == 2 ? 2 : 4));
        epi.count_planes = idx->ws_fany.as<uint32_t>();
    }
    epi.qf = idx->ws_fqf.as<float4>();
    epi.rowc = io.d_rowc; epi.qc = idx->ws_qc.as<orr::QueryConst>(); epi.kw = io.kw;
    epi.cnt = idx->ws_fcnt.as<uint32_t>(); epi.buf = idx->ws_fbuf.as<orr::SelEntry>(); epi.cap = kCap;
    // (the counters are cleared by the query-constants launch in front of the screening launches; the int8 stream cleared
    // them with the queries' images)
    if (p.screen == Screen::GemvBf16) HIP_TRY(hipMemsetAsync(idx->ws_fcnt.p, 0, sizeof(uint32_t) * 3 * (size_t)B, s));
    ORR_TRY(idx->ws_tickets.reserve(sizeof(uint32_t) * 8 * 16));
    if (p.two_stage()) return screen_two_stage(idx, a, p, kprime, n, io, epi, kCap, buf_lists, lists_total, host_records, rec_bytes);

    {
        Timed t(idx, "select_floor", 0.0);
        HIP_TRY(orr::launch_select_final_sample(idx->ws_sel.as<orr::SelEntry>(), lists_total, fss, B, kprime, d_tau, s));
    }
    HIP_TRY(orr::launch_fused_query_consts(idx->ws_qc.as<orr::QueryConst>(), d_tau, B, idx->ws_fqf.as<float4>(), s, nullptr, nullptr, nullptr,
                                           idx->ws_fcnt.as<uint32_t>(), 3 * B));
    epi.tau = d_tau;
    {
        Timed t(idx, "gemm_dot_bf16x3_fused", 4.0 * (double)(n - p.dotf_rows) * idx->dim + 4.0 * (double)B * idx->dim);
        HIP_TRY(orr::launch_gemm_dot_bf16x3(idx->ws_qsplit.p, B, idx->d_emb, p.dotf_rows, n, idx->dim, nullptr, 0, &epi, 3, s));
    }
    {
        Timed t(idx, "buffer_to_lists", 0.0);
        HIP_TRY(orr::launch_buffer_to_lists(epi.buf, epi.cnt, kCap, B, fss, lists_total, idx->ws_sel.as<orr::SelEntry>(), s));
    }
    Timed t(idx, "select_final", (double)B * (double)lists_total * orr::kSelWidth * sizeof(orr::SelEntry));
    HIP_TRY(orr::launch_select_final(idx->ws_sel.as<orr::SelEntry>(), lists_total, B, kprime, n, idx->row_base,
                                     nullptr, nullptr, 0, idx->d_norm_b, idx->d_created, idx->d_row_ids, io.kw,
                                     0, p.approx_eps, nullptr, epi.cnt, kCap, nullptr, io.d_cand, s));
    return ORR_OK;
}

// Stage 7: selection for the form, then (batched pass) the records' dots again in the reference's own arithmetic (K6).  The
// Exact, StreamMfma and SplitAll forms score and select over every row; large batches scan a prefix first, take its k'-th
// best key per query as a floor, and let the rest of the corpus skip every 64-row batch that cannot beat it.
int launch_selection(orr_index *idx, const BatchArgs &a, const PassPlan &p, int32_t kprime, int64_t n, PassIo &io, bool host_records,
                     size_t rec_bytes)
{
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    if (p.form == PassForm::LargeK)
        return run_large_k(idx, a, kprime, n, io.d_dot, io.kw, idx->pin_qc.as<orr::QueryConst>(), io.d_cand, s);
    const int64_t n_seg = (n + orr::kSelSegRows - 1) / orr::kSelSegRows;
    const int32_t n_seg32 = (int32_t)n_seg;
    ORR_TRY(idx->ws_sel.reserve(sizeof(orr::SelEntry) * (size_t)B * (size_t)n_seg * orr::kSelWidth));
    if (p.fused()) {
        ORR_TRY(select_fused(idx, a, p, kprime, n, io, host_records, rec_bytes));
    } else {
        const orr::QueryConst *qc = idx->ws_qc.as<orr::QueryConst>();
        unsigned long long *d_tau = nullptr;
        const int32_t sample_seg = (B >= 8 && n_seg32 >= 48) ? std::min<int32_t>(64, std::max<int32_t>(16, n_seg32 / 16)) : 0;
        if (sample_seg > 0) {
            ORR_TRY(idx->ws_tau.reserve(sizeof(unsigned long long) * (size_t)B));
            d_tau = idx->ws_tau.as<unsigned long long>();
            {
                Timed t(idx, "fuse_select", (double)B * (double)sample_seg * orr::kSelSegRows * 28.0);
                HIP_TRY(orr::launch_fuse_select(io.d_dot, io.d_dotf, n, idx->d_norm_b, idx->d_created, io.d_rowc, io.kw, qc, a.now_ticks,
                                                n, B, 0, sample_seg, nullptr, idx->ws_sel.as<orr::SelEntry>(), 0, s));
            }
            Timed t(idx, "select_floor", 0.0);
            HIP_TRY(orr::launch_select_final_sample(idx->ws_sel.as<orr::SelEntry>(), n_seg32, sample_seg, B, kprime, d_tau, s));
        }
        {
            Timed t(idx, "fuse_select", (double)B * (double)n * (8.0 * (p.use_cos ? 1 : 0) + 8.0 + 8.0));
            HIP_TRY(orr::launch_fuse_select(io.d_dot, io.d_dotf, n, idx->d_norm_b, idx->d_created, io.d_rowc, io.kw, qc, a.now_ticks,
                                            n, B, sample_seg, n_seg32 - sample_seg, d_tau, idx->ws_sel.as<orr::SelEntry>(), 0, s));
        }
        Timed t(idx, "select_final", (double)B * (double)n_seg * orr::kSelWidth * sizeof(orr::SelEntry));
        HIP_TRY(orr::launch_select_final(idx->ws_sel.as<orr::SelEntry>(), n_seg32, B, kprime, n, idx->row_base,
                                         io.d_dot, io.d_dotf, n, idx->d_norm_b, idx->d_created, idx->d_row_ids, io.kw,
                                         p.use_mfma ? 0 : 1, p.approx_eps, nullptr, nullptr, 0u, nullptr, io.d_cand, s));
    }
    if (p.use_mfma && !p.two_stage()) {
        Timed t(idx, "rescore_exact", (double)B * kprime * 4.0 * idx->dim);
        HIP_TRY(orr::launch_rescore_exact(idx->d_emb, idx->dim, io.d_q, B, kprime, idx->row_base, io.d_cand, s));
    }
    return ORR_OK;
}

// What the keyword chain leaves behind, put right for the next chain on this lane: the term bitmaps it used cleared, its
// counters zeroed.  Every kernel that read the bitmaps must be DONE (the host has waited for it): the large clear runs on the
// auxiliary stream, behind nothing.  finish_pass and orr_scope_create_terms both end with this.  (A chain whose caller skipped
// it clears everything itself, in front of its kernels: launch_keyword_side withdraws these vouchers on entry.)
int clean_keyword_side(orr_index *idx, const KwSide &kws, uint32_t n_terms_total)
{
    if (kws.bm_bytes) {        // every kernel that read the bitmaps is done: clear them for the next search
        const bool on_aux = kws.bm_bytes >= ((size_t)16 << 20);   // (small ones stay on the keyword stream: a cross-stream wait costs a one-query call more)
        if (on_aux) {
            HIP_TRY(hipMemsetAsync(idx->ws_bitmaps.p, 0, kws.bm_bytes, idx->stream_aux));
            HIP_TRY(hipEventRecord(idx->ev_bm_clean, idx->stream_aux));
        } else {
            HIP_TRY(hipMemsetAsync(idx->ws_bitmaps.p, 0, kws.bm_bytes, idx->stream_kw));
        }
        idx->kw_clean.grant_bitmaps(idx->ws_bitmaps.p, std::max(kws.bm_bytes, kws.bm_clean_before), on_aux);
    }
    if (n_terms_total > 0 && idx->ws_counter.p) {   // ... and the keyword chain's counters (two memsets less in front of the next chain)
        HIP_TRY(hipMemsetAsync(idx->ws_counter.p, 0, sizeof(unsigned long long), idx->stream_kw));
        if (idx->ws_kwalias.p) HIP_TRY(hipMemsetAsync(idx->ws_kwalias.p, 0, idx->ws_kwalias.cap, idx->stream_kw));
        idx->kw_clean.grant_counters(idx->ws_counter.p, idx->ws_kwalias.p);
    }
    return ORR_OK;
}

// The one rule for a hit list that may have been too short (keyword::after_run), behind the caller's synchronise: the count as
// expand_hits left it in pinned memory (the device copy is zeroed again behind the chain).  More hits than the list holds -- short
// terms against a large vocabulary -- and the bitmaps are incomplete: what was made of them is discarded, the lane keeps a list
// grown to the measured count and the chain runs again (kRetryPass); the callers' loops end after kMaxRuns runs.  fn: the entry point's
// name in front of the message, null for a search.
int check_hit_list(orr_index *idx, const KwSide &kws, const char *fn)
{
    if (!kws.overflow_possible) return ORR_OK;
    const uint32_t hits = (uint32_t)(*idx->pin_kwcnt.as<unsigned long long>() >> 32);
    const keyword::AfterRun r = keyword::after_run(hits, kws.max_hits);
    if (r.kind == keyword::AfterRun::Stands) return ORR_OK;
    if (r.kind == keyword::AfterRun::Refused)
        return fn ? fail(ORR_ENOMEM, "%s: the terms matched %u vocabulary tokens: a hit list of that size is refused (8 GiB)", fn, hits)
                  : fail(ORR_ENOMEM, "keyword terms matched %u vocabulary tokens: a hit list of that size is refused (8 GiB)", hits);
    idx->kw_hits_cap = r.new_cap;
    return kRetryPass;
}
int hit_list_kept_overflowing(const char *fn)
{
    return fn ? fail(ORR_EDEVICE, "%s: the keyword hit list kept overflowing", fn) : fail(ORR_EDEVICE, "the keyword hit list kept overflowing");
}

// Stage 9: wait for the pass; clear the keyword side's bitmaps and counters for the next search; statistics.  kRetryPass:
// the keyword hit list was too short and has grown, this pass's records are discarded.
int finish_pass(orr_index *idx, const BatchArgs &a, const PassPlan &p, const KwSide &kws, uint32_t n_terms_total)
{
    const int32_t B = a.B;
    HIP_TRY(hipStreamSynchronize(idx->stream));
    ORR_TRY(clean_keyword_side(idx, kws, n_terms_total));
    if (p.dev_norms) memcpy(idx->h_norm_a.data(), idx->pin_norm.p, sizeof(double) * (size_t)B);
    if (n_terms_total > 0) {
        idx->sstats.kw_hits_total += (int64_t)(*idx->pin_kwcnt.as<unsigned long long>() >> 32);
        idx->sstats.kw_passes += 1;
    }
    if (p.two_stage()) {
        idx->h_survivors.assign(idx->pin_cnt.as<uint32_t>(), idx->pin_cnt.as<uint32_t>() + B);
        uint64_t sum = 0;
        for (uint32_t cnt : idx->h_survivors) sum += cnt;
        const uint64_t mean = p.masked ? 1024 : sum / (uint64_t)B;     // (a masked pass has no sampled prefix to steer)
        if (mean > 4096 && idx->sample_boost < 16) idx->sample_boost *= 2;
        else if (mean < 512 && idx->sample_boost > 1) idx->sample_boost /= 2;
    }
    g_ht.mark(4);
    collect_events(idx);
    return check_hit_list(idx, kws, nullptr);
}

// Device side of one batch: exact dots, keyword bitmaps, fused scores, selection.
// Records ([B][kprime+1]) land in pinned host memory (*recs_host) when host_records is set
// and they are small, otherwise in idx->ws_cand (*recs_host = nullptr).  *q_host points at
// the query vectors in host memory (valid until the next call).  Caller holds the lock.
int run_shard_once(orr_index *idx, const BatchArgs &a, int32_t kprime, bool host_records, const float **q_host,
                   const orr_candidate **recs_host, PassPlan &p)
{
    g_ht.start();
    ORR_TRY(bind_device(idx));
    const int64_t n = participating_rows(idx, a.candidate_limit);
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    if (recs_host) *recs_host = nullptr;

    // ---- 1, 2. term offsets, the plan, record destination, query vectors
    PassFront f;
    ORR_TRY(open_pass(idx, a, kprime, [&](const std::vector<uint32_t> &qoff, PassPlan &plan) { return plan_pass(idx, a, kprime, n, qoff, plan); },
                      host_records, true, true, q_host, p, f));
    PassIo &io = f.io;

    if (p.form == PassForm::Empty) {   // nothing on this shard takes part: empty records + trailers
        const std::vector<orr_candidate> empty = empty_records(B, kprime);
        if (io.direct_host) memcpy(io.d_cand, empty.data(), f.rec_bytes);
        else HIP_TRY(hipMemcpyAsync(io.d_cand, empty.data(), f.rec_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (f.q_download_pending || p.dev_norms) HIP_TRY(hipEventSynchronize(idx->ev_q));    // nothing reads the caller's vectors after the call
        if (recs_host && io.direct_host) *recs_host = io.d_cand;
        return ORR_OK;
    }

    // ---- 3. the int8 image of 1..4 queries on the int8 shadow: the first thing the main stream needs, dependent on nothing
    // else, so that launch goes out before the host prepares the keyword side
    if (p.screen == Screen::GemvI8) ORR_TRY(launch_i8_query_image(idx, io.d_q, B, false, s));

    // ---- 4. K3 keyword side, on its own stream
    KwSide kws;
    ORR_TRY(launch_keyword_side(idx, a, f.qoff, kws));
    io.kw = kws.view;
    g_ht.mark(1);

    // ---- 5. cosine numerators
    ORR_TRY(launch_numerators(idx, a, p, n, io));
    g_ht.mark(0);

    // ---- 6. query constants and row constants, then the keyword side joins the main stream
    ORR_TRY(launch_consts(idx, a, p, n, f.qoff, f.q_download_pending, io));
    if (f.n_terms_total > 0) HIP_TRY(hipStreamWaitEvent(s, idx->ev_kw_done, 0));
    g_ht.mark(2);

    // ---- 7. K4/K5 fused score + selection for the form
    ORR_TRY(launch_selection(idx, a, p, kprime, n, io, host_records, f.rec_bytes));

    // ---- 8. records of deleted rows are dropped by the host finish; large record sets go into pinned memory in one copy
    if (!owner_of(idx)->dead.empty())
        HIP_TRY(orr::launch_mark_dead_records(io.d_cand, B, kprime, owner_of(idx)->d_dead.as<int64_t>(),
                                              (int32_t)owner_of(idx)->dead.size(), idx->row_base, s));
    if (host_records) ORR_TRY(records_to_host(idx, f, s));
    g_ht.mark(3);
    idx->sstats.pass_mode = p.pass_mode();

    // ---- 9. synchronise, clean up, statistics
    const int r = finish_pass(idx, a, p, kws, f.n_terms_total);
    if (r != ORR_OK) return r;
    if (recs_host && io.direct_host) *recs_host = io.d_cand;
    else if (recs_host && host_records) *recs_host = idx->pin_cand.as<orr_candidate>();
    return ORR_OK;
}

// A pass until the keyword hit list held every hit.  sstats.passes counts the attempts that were thrown away; the one that
// stood is the caller's to count.
template <class Pass>
int retry_pass(orr_index *idx, Pass &&once)
{
    for (int attempt = 0;; ++attempt) {
        const int r = once();
        if (r != kRetryPass) return r;
        idx->sstats.passes += 1;
        if (attempt + 1 >= keyword::kMaxRuns) return hit_list_kept_overflowing(nullptr);
    }
}

int run_shard(orr_index *idx, const BatchArgs &a, int32_t kprime, bool host_records, const float **q_host,
              const orr_candidate **recs_host, PassPlan &pass)
{
    // (the plan is made again: sample_boost may have changed)
    return retry_pass(idx, [&] { return run_shard_once(idx, a, kprime, host_records, q_host, recs_host, pass); });
}

// The ranking order of the host finish.
bool ranks_before(const Ranked &x, const Ranked &y)
{
    const int c = compare_double(x.score, y.score);
    if (c != 0) return c > 0;                 // OrderByDescending(score)       :34
    return x.order_key < y.order_key;         // ThenByDescending(created), stable == candidate order  :35
}

// Host finish for one query over records from any number of shards.
// Returns the number of results; *certified tells whether rows outside the
// candidate sets were provably unable to reach the top-k.
int32_t finish_query(const orr_candidate *const *shard_recs, int32_t n_shards, int32_t kprime, bool use_cos,
                     double norm_a, int32_t n_terms, int64_t now_ticks, int32_t topk, int64_t *out_rows,
                     double *out_scores, bool *certified, int *err, int64_t *out_keys = nullptr)
{
    std::vector<Ranked> ranked;
    double cutoff = -std::numeric_limits<double>::infinity();
    double eps = kCertifyEps;
    bool any_cut = false, overflow = false;
    double need_score = -std::numeric_limits<double>::infinity();   // two-stage: rows never offered score below this
    *err = ORR_OK;
    for (int32_t sidx = 0; sidx < n_shards; ++sidx) {
        const orr_candidate *rec = shard_recs[sidx];
        const orr_candidate &tr = rec[kprime];
        if (!(tr.flags & ORR_CAND_TRAILER) || tr.matches < 0 || tr.matches > kprime) {
            *err = fail(ORR_ECOMM, "orr_merge_candidates: shard %d has a malformed trailer", sidx);
            return 0;
        }
        for (int32_t i = 0; i < tr.matches; ++i) {
            const orr_candidate &c = rec[i];
            if (c.row_id < 0 && c.order_key < 0) continue;
            if (c.flags & ORR_CAND_DEAD) continue;                    // deleted row (orr_index_delete_rows)
            Ranked r;
            r.score = exact_score(c, use_cos, norm_a, n_terms, now_ticks);
            r.order_key = c.order_key;
            r.row_id = c.row_id;
            ranked.push_back(r);
        }
        if (tr.dot > eps) eps = tr.dot;            // bound of the pass that produced this shard's records
        if (tr.flags & ORR_CAND_OVERFLOW) overflow = true;
        if ((tr.flags & ORR_CAND_TWO_STAGE) && tr.norm_b > need_score) need_score = tr.norm_b;
        if (tr.approx_score != -std::numeric_limits<double>::infinity()) {
            any_cut = true;
            // NaN cut-off: the worst kept key was a NaN score, so everything left out is NaN too (NaN sorts last), harmless.
            // A list that pairs kept whatever their score filled to the brim reports +inf instead (cutoff_of_key): what was
            // left out is unknown there, no k-th score exceeds that cut-off, and the query climbs the ladder.
            if (!(tr.approx_score != tr.approx_score) && tr.approx_score > cutoff) cutoff = tr.approx_score;
        }
    }
    std::sort(ranked.begin(), ranked.end(), ranks_before);
    const int32_t take = std::max<int32_t>(1, topk);                                 // :36
    const int32_t n_out = (int32_t)std::min<size_t>((size_t)take, ranked.size());
    for (int32_t i = 0; i < n_out; ++i) {
        out_rows[i] = ranked[i].row_id;
        out_scores[i] = ranked[i].score;
        if (out_keys) out_keys[i] = ranked[i].order_key;
    }
    const bool lower_bounded = need_score != -std::numeric_limits<double>::infinity();
    if (overflow) {
        *certified = false;                       // some survivors were dropped: repeat unfused
    } else if (!any_cut && !lower_bounded) {
        *certified = true;
    } else if (n_out < take) {
        *certified = false;                       // fewer results than asked while rows were cut
    } else {
        const double sk = ranked[n_out - 1].score;
        *certified = !any_cut || sk > cutoff + eps;           // false for NaN
        // two-stage: rows that were never offered score below need_score, and the construction makes
        // S_k >= need_score; a violated bound must not pass silently
        if (*certified && lower_bounded) *certified = sk >= need_score - 1e-12;
    }
    return n_out;
}

int merge_impl(int32_t n_shards, int32_t B, int32_t kprime, const orr_candidate *all, int32_t dim, bool use_cos,
               const float *q_host, const double *norms, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
               int64_t *out_rows, double *out_scores, int32_t *out_counts, int32_t *out_uncertified,
               uint8_t *out_certified = nullptr, int64_t *out_keys = nullptr)
{
    const int32_t take = std::max<int32_t>(1, topk);
    int32_t unc = 0;
    std::vector<double> own_norms;
    if (use_cos && !norms) {
        own_norms.resize((size_t)B);
        exact_norms(q_host, B, dim, own_norms.data());
        norms = own_norms.data();
    }
    // queries are independent: large merges (many queries x many shards) are split over a few host threads
    auto work = [&](int32_t b_begin, int32_t b_end, int32_t *unc_out, int *err_out) {
        std::vector<const orr_candidate *> recs((size_t)n_shards);
        for (int32_t b = b_begin; b < b_end; ++b) {
            for (int32_t sidx = 0; sidx < n_shards; ++sidx)
                recs[sidx] = all + ((size_t)sidx * B + b) * ((size_t)kprime + 1);
            const double norm_a = use_cos ? norms[b] : 0.0;
            const int32_t n_terms = (int32_t)(query_term_off[b + 1] - query_term_off[b]);
            bool cert = false;
            int err = ORR_OK;
            for (int32_t i = 0; i < take; ++i) { out_rows[(size_t)b * take + i] = -1; out_scores[(size_t)b * take + i] = 0.0; }
            const int32_t cnt = finish_query(recs.data(), n_shards, kprime, use_cos, norm_a, n_terms, now_ticks, topk,
                                             out_rows + (size_t)b * take, out_scores + (size_t)b * take, &cert, &err,
                                             out_keys ? out_keys + (size_t)b * take : nullptr);
            if (err != ORR_OK) { *err_out = err; return; }
            if (out_counts) out_counts[b] = cnt;
            if (out_certified) out_certified[b] = cert ? 1 : 0;
            if (!cert) ++*unc_out;
        }
    };
    const int64_t n_records = (int64_t)B * n_shards * kprime;
    int n_thr = n_records >= 4096 ? std::min(HostPool::get().width() * 2, (B + 15) / 16) : 1;     // tasks of >= 16 queries
    if (n_thr < 1) n_thr = 1;
    std::vector<int32_t> t_unc((size_t)n_thr, 0);
    std::vector<int> t_err((size_t)n_thr, ORR_OK);
    if (n_thr == 1) {
        work(0, B, &t_unc[0], &t_err[0]);
    } else {
        HostPool::get().run(n_thr, [&](int t) {
            work((int32_t)((int64_t)B * t / n_thr), (int32_t)((int64_t)B * (t + 1) / n_thr), &t_unc[(size_t)t], &t_err[(size_t)t]);
        });
    }
    for (int t = 0; t < n_thr; ++t) {
        if (t_err[(size_t)t] != ORR_OK)
            return n_thr == 1 ? t_err[0] : fail(t_err[(size_t)t], "orr_merge_candidates: a shard's records are malformed");   // the detail was set on a pool thread
        unc += t_unc[(size_t)t];
    }
    if (out_uncertified) *out_uncertified = unc;
    return ORR_OK;
}

// Host finish of one pass over the sub-batch `cur` = queries `ids` of the call: the results go to out_*[ids[i]] of the call's
// numbering, cert[i] tells whether query i of the sub-batch was certified.
int merge_into(int32_t n_shards, int32_t kprime, const orr_candidate *recs, const BatchArgs &cur, bool use_cos, const float *q_host,
               const double *norms, const std::vector<int32_t> &ids, int64_t *out_rows, double *out_scores, int32_t *out_counts,
               std::vector<uint8_t> &cert)
{
    const int32_t nb = (int32_t)ids.size(), take = std::max<int32_t>(1, cur.topk);
    cert.assign((size_t)nb, 1);
    std::vector<int64_t> rows((size_t)nb * take);
    std::vector<double> scores((size_t)nb * take);
    std::vector<int32_t> counts((size_t)nb);
    std::vector<int64_t> keys(cur.out_keys ? (size_t)nb * take : 0);
    ORR_TRY(merge_impl(n_shards, nb, kprime, recs, cur.dim, use_cos, q_host, norms, cur.query_term_off, cur.now_ticks, cur.topk, rows.data(),
                       scores.data(), counts.data(), nullptr, cert.data(), cur.out_keys ? keys.data() : nullptr));
    for (int32_t i = 0; i < nb; ++i) {
        const size_t b = (size_t)ids[(size_t)i];
        if (cur.out_keys) memcpy(cur.out_keys + b * take, keys.data() + (size_t)i * take, sizeof(int64_t) * take);
        memcpy(out_rows + b * take, rows.data() + (size_t)i * take, sizeof(int64_t) * take);
        memcpy(out_scores + b * take, scores.data() + (size_t)i * take, sizeof(double) * take);
        if (out_counts) out_counts[b] = counts[(size_t)i];
    }
    return ORR_OK;
}

// ---- one batch through the passes, escalating ONLY the queries that could not be certified ----------------------------
// A query whose top-k could not be certified (a tie at the cut, a survivors' buffer that overflowed, k' too small for a
// mass of equal scores) goes through the next more exact pass as part of a compacted sub-batch; the others keep their
// results.  Which pass that is, and that the ladder ends, is orr_escalation.h's; escalate() below runs it for one index and
// for the shards of a cluster.

struct SubBatch {                  // storage of a compacted sub-batch (the vectors live in idx->ws_qsub when they are device-resident)
    std::vector<float> q_host;
    std::vector<uint8_t> pool;
    std::vector<uint32_t> term_off, qoff;
    std::vector<double> norms;
};

// The queries `ids` of `orig` as a batch of their own: `orig` itself where that is all of them in order.
int build_subset(orr_index *idx, const BatchArgs &orig, const std::vector<int32_t> &ids, SubBatch &sb, BatchArgs &out)
{
    out = orig;
    const int32_t nb = (int32_t)ids.size();
    bool whole = nb == orig.B;
    for (int32_t i = 0; i < nb && whole; ++i) whole = ids[(size_t)i] == i;
    if (whole) return ORR_OK;
    out.B = nb;
    if (orig.norms_host) {                             // (per query of the batch, as the vectors are)
        sb.norms.resize((size_t)nb);
        for (int32_t i = 0; i < nb; ++i) sb.norms[(size_t)i] = orig.norms_host[ids[(size_t)i]];
        out.norms_host = sb.norms.data();
    }
    if (orig.dim > 0) {
        const size_t row = (size_t)orig.dim;
        if (is_device_pointer(orig.q)) {
            ORR_TRY(idx->ws_qsub.reserve(sizeof(float) * row * (size_t)nb));
            for (int32_t i = 0; i < nb; ++i)
                HIP_TRY(hipMemcpyAsync(idx->ws_qsub.as<float>() + (size_t)i * row, orig.q + (size_t)ids[(size_t)i] * row, sizeof(float) * row,
                                       hipMemcpyDeviceToDevice, idx->stream));
            HIP_TRY(hipStreamSynchronize(idx->stream));
            out.q = idx->ws_qsub.as<float>();
        } else {
            sb.q_host.resize(row * (size_t)nb);
            for (int32_t i = 0; i < nb; ++i)
                memcpy(sb.q_host.data() + (size_t)i * row, orig.q + (size_t)ids[(size_t)i] * row, sizeof(float) * row);
            out.q = sb.q_host.data();
        }
    }
    sb.pool.clear(); sb.term_off.assign(1, 0u); sb.qoff.assign(1, 0u);
    for (int32_t i = 0; i < nb; ++i) {
        const int32_t b = ids[(size_t)i];
        for (uint32_t t = orig.query_term_off[b]; t < orig.query_term_off[b + 1]; ++t) {
            const uint32_t o = orig.term_off[t], e = orig.term_off[t + 1];
            if (e < o) return fail(ORR_EINVAL, "term_off is not monotone at term %u", t);
            sb.pool.insert(sb.pool.end(), orig.terms_utf8 + o, orig.terms_utf8 + e);
            sb.term_off.push_back((uint32_t)sb.pool.size());
        }
        sb.qoff.push_back((uint32_t)sb.term_off.size() - 1u);
    }
    sb.pool.push_back(0);
    out.terms_utf8 = sb.pool.data();
    out.term_off = sb.term_off.data();
    out.query_term_off = sb.qoff.data();
    return ORR_OK;
}

using escalation::ShardOutcome;

ShardOutcome outcome_of(const orr_index *lane, const PassPlan &pass, int64_t n)       // caller holds the lane
{
    ShardOutcome o;
    o.two_stage = pass.two_stage(); o.fused = pass.fused(); o.use_mfma = pass.use_mfma;
    o.pass_cap = lane->pass_cap; o.survivor_cap = lane->survivor_cap;
    o.n = n;
    o.pass_mode = lane->sstats.pass_mode;
    o.survivors = lane->h_survivors;
    return o;
}

// What one pass over a (sub-)batch hands to the host finish: the records of every shard, [G][B][k'+1], and what the shards kept.
struct PassResult {
    std::vector<ShardOutcome> shards;
    const orr_candidate *recs = nullptr;
    const float *q_host = nullptr;      // the query vectors in host memory, or null where norms are given and suffice
    const double *norms = nullptr;      // exact norms of the queries (cosine only)
    std::vector<orr_candidate> rec_store;
    std::vector<double> norm_store;
};

// How escalate() reaches the GPU: one index on the lane its caller holds, or the shards of a cluster.
struct Backend {
    const char *name;                   // for messages
    int32_t dim;
    orr_index *subset_on;               // whose workspace holds a sub-batch of device-resident query vectors (build_subset)
    int64_t n_total;                    // participating rows, all shards
    int64_t slice_rows;                 // ... of the largest shard: what a per-(query,row) workspace is sized by
    bool repeat_only_if_grown;          // escalation::decide
    orr_search_stats *stats;
    std::mutex *stats_mu;               // null: the caller's lock covers `stats`
    std::function<int(const BatchArgs &, int32_t kprime, PassResult &)> run_pass;
    std::function<void(const std::vector<ShardOutcome> &, const std::vector<uint32_t> &new_cap)> grow;   // GrowBuffers: Decision::new_cap
};

// One batch through the passes until every query is certified or nothing more exact exists.  Results go to out_*[b] of the
// batch's numbering; a repeat overwrites what its pass could not certify.
int escalate(const Backend &be, const BatchArgs &orig, int64_t kprime, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    struct Rung {                       // queries of `orig` (ascending) and the pass they go through next
        std::vector<int32_t> ids;
        bool no_fuse, force_exact;
        int64_t kprime;
        int repeats;
    };
    const bool use_cos = orig.dim > 0 && orig.dim == be.dim;
    std::deque<Rung> todo(1, Rung{std::vector<int32_t>((size_t)orig.B), orig.no_fuse, orig.force_exact, kprime, 0});
    std::iota(todo.front().ids.begin(), todo.front().ids.end(), 0);
    while (!todo.empty()) {            // depth first: a slice's repeats run before the next slice
        const Rung r = std::move(todo.front());
        todo.pop_front();
        const int32_t nb = (int32_t)r.ids.size();
        if (const int32_t per = escalation::slice_width(nb, be.slice_rows, r.no_fuse || r.force_exact)) {
            for (int32_t i0 = (nb - 1) / per * per; i0 >= 0; i0 -= per)
                todo.push_front(Rung{std::vector<int32_t>(r.ids.begin() + i0, r.ids.begin() + std::min<int32_t>(nb, i0 + per)),
                                     r.no_fuse, r.force_exact, r.kprime, r.repeats});
            continue;
        }
        SubBatch sb;
        BatchArgs cur;
        ORR_TRY(build_subset(be.subset_on, orig, r.ids, sb, cur));
        cur.no_fuse = r.no_fuse; cur.force_exact = r.force_exact;
        PassResult pr;
        ORR_TRY(be.run_pass(cur, (int32_t)r.kprime, pr));
        std::vector<uint8_t> cert;
        ORR_TRY(merge_into((int32_t)pr.shards.size(), (int32_t)r.kprime, pr.recs, cur, use_cos, pr.q_host, pr.norms, r.ids, out_rows, out_scores,
                           out_counts, cert));
        g_ht.mark(5);
        const escalation::Decision d = escalation::decide(pr.shards, cert, r.no_fuse, r.force_exact, r.kprime, be.n_total, be.repeat_only_if_grown);
        {
            std::unique_lock<std::mutex> lock = be.stats_mu ? std::unique_lock<std::mutex>(*be.stats_mu) : std::unique_lock<std::mutex>();
            orr_search_stats &s = *be.stats;
            s.passes += 1;
            s.pass_mode = pr.shards[0].pass_mode;
            if (r.repeats > 0) s.requeried += nb;
            for (const ShardOutcome &o : pr.shards) escalation::account_survivors(s, o, (size_t)nb);
            if (d.step == escalation::Step::GrowBuffers) s.buffer_growths += 1;
            if (d.step == escalation::Step::Exact) s.exact_pass_queries += (int64_t)d.again.size();
        }
        if (d.again.empty()) continue;
        if (r.repeats >= escalation::kMaxRepeats) return fail(ORR_EDEVICE, "%s: escalation did not terminate", be.name);
        Rung next{{}, r.no_fuse, r.force_exact, d.kprime, r.repeats + 1};
        for (int32_t i : d.again) next.ids.push_back(r.ids[(size_t)i]);
        if (d.step == escalation::Step::GrowBuffers) be.grow(pr.shards, d.new_cap);
        if (d.step == escalation::Step::Unfused) next.no_fuse = true;
        if (d.step == escalation::Step::Exact) next.force_exact = true;
        todo.push_front(std::move(next));
    }
    return ORR_OK;
}

// escalate() on one index: the passes run on the lane the caller holds (under its lock).
Backend index_backend(orr_index *idx, const char *name, int64_t n)
{
    Backend be{name, idx->dim, idx, n, n, false, &idx->sstats, nullptr, nullptr, nullptr};
    be.run_pass = [idx, n](const BatchArgs &cur, int32_t kprime, PassResult &pr) -> int {
        PassPlan pass;
        ORR_TRY(run_shard(idx, cur, kprime, true, &pr.q_host, &pr.recs, pass));
        if (!pr.recs) {                               // large record sets stay on the device until here
            pr.rec_store.resize((size_t)cur.B * ((size_t)kprime + 1));
            HIP_TRY(hipMemcpy(pr.rec_store.data(), idx->ws_cand.p, sizeof(orr_candidate) * pr.rec_store.size(), hipMemcpyDeviceToHost));
            pr.recs = pr.rec_store.data();
        }
        pr.norms = idx->h_norm_a.data();
        pr.shards.assign(1, outcome_of(idx, pass, n));
        return ORR_OK;
    };
    // the index keeps the larger size for later searches, and the other lanes of the handle start from it as well (a view the
    // caller made tells its parent nothing)
    be.grow = [idx](const std::vector<ShardOutcome> &, const std::vector<uint32_t> &new_cap) {
        if (new_cap[0] > idx->survivor_cap) idx->survivor_cap = new_cap[0];
        if (!idx->is_view || idx->internal_lane) publish_survivor_hint(const_cast<orr_index *>(owner_of(idx)), new_cap[0]);
    };
    return be;
}

// ---- scoped search: rank only the rows a caller lists (orr_search_batch_scoped, orr_search_shard_scoped) -------------------
// Query b's scope is a list of row ids.  The ids are resolved on the device (a table of the shard's (id, position) pairs sorted
// by id, a binary search per listed id) into one bitmap over the shard's rows per query -- repeats fall together, the bits are
// in candidate order, deleted rows are left out, candidate_limit is a prefix popcount -- and the bitmaps are compacted into the
// survivors' buffers of the two-stage pass, whose exact tail (two_stage_tail) then runs as behind a screen.  No screen, no
// shadow, no pass over all rows; the forms, the ladder and the slicing are orr_scope_plan.h's.

struct ScopeArgs {
    int64_t n_ids;
    const int64_t *ids;            // host or device
    const uint64_t *off;           // host [B + 1], or null: every query owns the whole list
    const int64_t *before;         // host [B] scoped live rows in the shards in front (orr_search_shard_scoped), or null
};

int check_scope_args(int32_t B, const ScopeArgs &sc, const char *fn)
{
    if (sc.n_ids < 0) return fail(ORR_EINVAL, "%s: n_scope_ids is negative", fn);
    if (sc.n_ids > 0 && !sc.ids) return fail(ORR_EINVAL, "%s: scope_ids is NULL with %lld ids", fn, (long long)sc.n_ids);
    if (B > 0 && !scope::offsets_valid(sc.off, B, sc.n_ids))
        return fail(ORR_EINVAL, "%s: scope_off must start at 0, never decrease and end at n_scope_ids", fn);
    return ORR_OK;
}

int check_scope(const orr_index *idx, int32_t B, const ScopeArgs &sc, const char *fn)
{
    ORR_TRY(check_scope_args(B, sc, fn));
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    return ORR_OK;
}

// The id table, once per sealed shard (12 bytes per row); the caller holds a lane of the handle.  ORR_ENOMEM without room.
int ensure_scope_table(orr_index *lane)
{
    orr_index *own = const_cast<orr_index *>(owner_of(lane));
    if (own->scope_ready.load(std::memory_order_acquire)) return ORR_OK;
    std::lock_guard<std::mutex> g(own->scope_mu);
    if (own->scope_ready.load(std::memory_order_acquire)) return ORR_OK;
    const int64_t n = own->n_rows;
    if (n > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        DevBuf iota, tmp;
        size_t tmp_bytes = 0;
        HIP_TRY(orr::scope_sort_id_table(nullptr, tmp_bytes, own->d_row_ids, nullptr, nullptr, nullptr, n, lane->stream));
        int64_t *ids = nullptr;
        uint32_t *pos = nullptr;
        int r = dev_alloc(&ids, (size_t)n);
        if (r == ORR_OK) r = dev_alloc(&pos, (size_t)n);
        if (r == ORR_OK) r = iota.reserve(sizeof(uint32_t) * (size_t)n);
        if (r == ORR_OK) r = tmp.reserve(tmp_bytes);
        if (r == ORR_OK) {
            size_t tb = tmp.cap;
            hipError_t e = orr::scope_sort_id_table(tmp.p, tb, own->d_row_ids, ids, iota.as<uint32_t>(), pos, n, lane->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(lane->stream);
            if (e != hipSuccess) r = fail(ORR_EDEVICE, "scope id table: %s", hipGetErrorString(e));
        }
        iota.release(); tmp.release();
        if (r != ORR_OK) {
            (void)hipGetLastError();
            if (ids) (void)hipFree(ids);
            if (pos) (void)hipFree(pos);
            return r;
        }
        own->scope_tab_ids = ids;
        own->scope_tab_pos = pos;
        add_phase_stat(lane, "scope_id_table", t0, 12.0 * (double)n);
    }
    own->scope_ready.store(true, std::memory_order_release);
    return ORR_OK;
}

// The scope bitmaps of queries [b0, b0 + nq) of a call, on the lane's workspaces, and what they resolve to.
struct ScopeSlice {
    int32_t b0 = 0, nq = 0, n_bitmaps = 0;
    int64_t words = 0;
    const uint32_t *live = nullptr;    // pinned host [nq]: live rows of each query's scope on this shard
    const uint32_t *took = nullptr;    // ... of which the first limit take part
    const int64_t *d_limit = nullptr;  // device [nq]
    const uint32_t *bm = nullptr;      // device [n_bitmaps][words]: the lane's ws_scope_bm, or a scope handle's own (read-only)
    const uint32_t *chunks = nullptr;  // device [n_bitmaps][scope_chunks(words)], likewise
};

// limit[b]: scoped live rows query b of the CALL lets take part.  Ends in a stream synchronise: live / took are final.
int build_scope_slice(orr_index *idx, const ScopeArgs &sc, const std::vector<int64_t> &limit, int32_t b0, int32_t nq, ScopeSlice &sl)
{
    hipStream_t s = idx->stream;
    const orr_index *own = owner_of(idx);
    const bool shared = sc.off == nullptr;
    const uint64_t id0 = shared ? 0 : sc.off[b0], id1 = shared ? (uint64_t)sc.n_ids : sc.off[b0 + nq];
    const int64_t n_ids = (int64_t)(id1 - id0);
    sl.b0 = b0; sl.nq = nq; sl.n_bitmaps = shared ? 1 : nq;
    sl.words = (int64_t)(scope::bitmap_bytes(idx->n_rows) / 4);
    const int32_t n_chunks = orr::scope_chunks(sl.words);
    // one pinned block: [offsets u64 x (nq + 1)][limits i64 x nq][live u32 x nq][took u32 x nq]; the first two go up
    const size_t o_lim = sizeof(uint64_t) * ((size_t)nq + 1), o_live = o_lim + sizeof(int64_t) * (size_t)nq, o_took = o_live + sizeof(uint32_t) * (size_t)nq;
    ORR_TRY(idx->pin_scope.reserve(o_took + sizeof(uint32_t) * (size_t)nq));
    ORR_TRY(idx->ws_scope_meta.reserve(o_live));
    ORR_TRY(idx->ws_scope_ids.reserve(sizeof(int64_t) * (size_t)std::max<int64_t>(n_ids, 1)));
    ORR_TRY(idx->ws_scope_bm.reserve(sizeof(uint32_t) * (size_t)sl.n_bitmaps * (size_t)sl.words));
    ORR_TRY(idx->ws_scope_chunks.reserve(sizeof(uint32_t) * (size_t)sl.n_bitmaps * (size_t)n_chunks));
    uint8_t *hp = idx->pin_scope.as<uint8_t>();
    uint64_t *h_off = reinterpret_cast<uint64_t *>(hp);
    int64_t *h_lim = reinterpret_cast<int64_t *>(hp + o_lim);
    for (int32_t i = 0; i <= nq; ++i) h_off[i] = shared ? 0 : sc.off[b0 + i] - id0;
    for (int32_t i = 0; i < nq; ++i) h_lim[i] = limit[(size_t)(b0 + i)];
    uint32_t *h_live = reinterpret_cast<uint32_t *>(hp + o_live), *h_took = reinterpret_cast<uint32_t *>(hp + o_took);
    uint8_t *dm = idx->ws_scope_meta.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(dm, hp, o_live, hipMemcpyHostToDevice, s));
    if (n_ids > 0) HIP_TRY(hipMemcpyAsync(idx->ws_scope_ids.p, sc.ids + id0, sizeof(int64_t) * (size_t)n_ids, hipMemcpyDefault, s));   // the list is copied, nothing else
    HIP_TRY(hipMemsetAsync(idx->ws_scope_bm.p, 0, sizeof(uint32_t) * (size_t)sl.n_bitmaps * (size_t)sl.words, s));
    sl.d_limit = reinterpret_cast<const int64_t *>(dm + o_lim);
    {
        Timed t(idx, "scope_lookup", 8.0 * (double)n_ids);
        HIP_TRY(orr::launch_scope_lookup(own->scope_tab_ids, own->scope_tab_pos, idx->n_rows, idx->ws_scope_ids.as<int64_t>(), n_ids,
                                         shared ? nullptr : reinterpret_cast<const uint64_t *>(dm), nq, own->d_dead.as<int64_t>(),
                                         (int32_t)own->dead.size(), idx->ws_scope_bm.as<uint32_t>(), sl.words, s));
    }
    {
        Timed t(idx, "scope_counts", 4.0 * (double)sl.n_bitmaps * (double)sl.words);
        HIP_TRY(orr::launch_scope_counts(idx->ws_scope_bm.as<uint32_t>(), sl.words, sl.n_bitmaps, nq, sl.d_limit, idx->ws_scope_chunks.as<uint32_t>(),
                                         h_live, h_took, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(idx);
    sl.live = h_live; sl.took = h_took;
    sl.bm = idx->ws_scope_bm.as<uint32_t>(); sl.chunks = idx->ws_scope_chunks.as<uint32_t>();
    return ORR_OK;
}

// The slice of a call whose B queries share the scope of a handle: nothing is resolved, the numbers are the handle's and the
// bitmap is the handle's own (a search never writes it: the list path writes its parts into the lane's workspace).  The caller
// holds the scope shared.  No synchronise: the limits go up in stream order.
int slice_of_handle(orr_index *idx, const orr_scope *h, int32_t B, int64_t limit_rows, ScopeSlice &sl)
{
    sl.b0 = 0; sl.nq = B; sl.n_bitmaps = 1; sl.words = h->words;
    const size_t o_lim = sizeof(uint64_t) * ((size_t)B + 1), o_live = o_lim + sizeof(int64_t) * (size_t)B, o_took = o_live + sizeof(uint32_t) * (size_t)B;
    ORR_TRY(idx->pin_scope.reserve(o_took + sizeof(uint32_t) * (size_t)B));      // build_scope_slice's block
    ORR_TRY(idx->ws_scope_meta.reserve(o_live));
    uint8_t *hp = idx->pin_scope.as<uint8_t>();
    uint64_t *h_off = reinterpret_cast<uint64_t *>(hp);
    int64_t *h_lim = reinterpret_cast<int64_t *>(hp + o_lim);
    uint32_t *h_live = reinterpret_cast<uint32_t *>(hp + o_live), *h_took = reinterpret_cast<uint32_t *>(hp + o_took);
    const int64_t live = h->live.load();
    for (int32_t i = 0; i <= B; ++i) h_off[i] = 0;
    for (int32_t i = 0; i < B; ++i) {
        h_lim[i] = limit_rows;
        h_live[i] = (uint32_t)live;
        h_took[i] = (uint32_t)std::min<int64_t>(live, std::max<int64_t>(0, limit_rows));
    }
    uint8_t *dm = idx->ws_scope_meta.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(dm, hp, o_live, hipMemcpyHostToDevice, idx->stream));
    sl.d_limit = reinterpret_cast<const int64_t *>(dm + o_lim);
    sl.live = h_live; sl.took = h_took;
    sl.bm = h->bm; sl.chunks = h->chunks;
    return ORR_OK;
}

// One scoped pass over the queries of `a` (a compacted sub-batch; query i of it is query qsel[i] of the slice): the slice's
// bitmaps -> survivors' buffers -> the exact tail (Selection) or every pair a record (AllRecords, kprime >= every count).  The
// records land in host memory (*recs_host).  kRetryPass as run_shard_once, whose front end and stages it runs in the same
// order without a screen.  Caller holds the lane and its lock.
int run_scoped_pass(orr_index *idx, const BatchArgs &a, const std::vector<uint32_t> &qsel, const ScopeSlice &sl, scope::Form form,
                    int32_t kprime, const float **q_host, const orr_candidate **recs_host)
{
    ORR_TRY(bind_device(idx));
    const int32_t B = a.B, D = idx->dim;
    hipStream_t s = idx->stream;
    *recs_host = nullptr;
    PassPlan p;
    PassFront f;
    auto plan = [&](const std::vector<uint32_t> &, PassPlan &pl) {   // what launch_consts and finish_pass read of a plan: no screen, no batched score
        pl.form = PassForm::Exact;
        pl.use_cos = a.dim > 0 && a.dim == D;
        pl.q_on_device = pl.use_cos && is_device_pointer(a.q);
        return ORR_OK;
    };
    ORR_TRY(open_pass(idx, a, kprime, plan, true, false, false, q_host, p, f));
    PassIo &io = f.io;

    // ---- the survivors' buffers, filled from the bitmaps: [counts | unused | tickets] as the tail expects them, no floor
    uint32_t worst = 0;
    for (uint32_t q : qsel) worst = std::max(worst, sl.took[q]);
    const uint32_t cap = scope::slice_cap(worst);
    const int32_t buf_lists = (int32_t)(cap / orr::kSelWidth);
    const size_t o_sel = sizeof(uint32_t) * 3 * (size_t)B, o_L = (o_sel + sizeof(uint32_t) * (size_t)B + 7) / 8 * 8;
    ORR_TRY(idx->pin_scope_pass.reserve(o_L + sizeof(double) * (size_t)B));
    uint8_t *hp = idx->pin_scope_pass.as<uint8_t>();
    uint32_t *h_cnt = reinterpret_cast<uint32_t *>(hp), *h_sel = reinterpret_cast<uint32_t *>(hp + o_sel);
    double *h_L = reinterpret_cast<double *>(hp + o_L);
    for (int32_t b = 0; b < B; ++b) {
        h_cnt[b] = sl.took[qsel[(size_t)b]]; h_cnt[B + b] = 0; h_cnt[2 * B + b] = 0;
        h_sel[b] = qsel[(size_t)b];
        h_L[b] = -std::numeric_limits<double>::infinity();
    }
    ORR_TRY(idx->ws_fcnt.reserve(o_sel));
    ORR_TRY(idx->ws_scope_sel.reserve(sizeof(uint32_t) * (size_t)B));
    ORR_TRY(idx->ws_tsL.reserve(sizeof(double) * (size_t)B));
    ORR_TRY(idx->ws_fbuf.reserve(sizeof(orr::SelEntry) * (size_t)B * cap));
    HIP_TRY(hipMemcpyAsync(idx->ws_fcnt.p, h_cnt, o_sel, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(idx->ws_scope_sel.p, h_sel, sizeof(uint32_t) * (size_t)B, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(idx->ws_tsL.p, h_L, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, s));
    orr::FusedEpilogue epi{};
    epi.cnt = idx->ws_fcnt.as<uint32_t>(); epi.buf = idx->ws_fbuf.as<orr::SelEntry>(); epi.cap = cap;
    {
        Timed t(idx, "scope_compact", 16.0 * (double)B * (double)worst);
        HIP_TRY(orr::launch_scope_compact(sl.bm, sl.words, sl.n_bitmaps, sl.chunks, idx->ws_scope_sel.as<uint32_t>(), B, sl.d_limit, epi.buf, cap, s));
    }

    // ---- keyword side (its own stream), query constants, then the two join
    KwSide kws;
    ORR_TRY(launch_keyword_side(idx, a, f.qoff, kws));
    io.kw = kws.view;
    ORR_TRY(launch_consts(idx, a, p, 0, f.qoff, f.q_download_pending, io));
    if (f.n_terms_total > 0) HIP_TRY(hipStreamWaitEvent(s, idx->ev_kw_done, 0));

    // ---- the re-score in the reference arithmetic and the records
    const Rescore how = p.use_cos && D % 64 == 0 ? Rescore::BufferExact : Rescore::ScopeGeneric;
    const double pair_bytes = (double)B * (double)worst * 4.0 * (p.use_cos ? D : 0);
    if (form == scope::Form::AllRecords) {
        ORR_TRY(idx->ws_fdot.reserve(sizeof(double) * (size_t)B * cap));
        ORR_TRY(rescore_survivors(idx, a, io, epi, cap, how, pair_bytes, s));
        Timed t(idx, "scope_records", (double)f.rec_bytes);
        HIP_TRY(orr::launch_scope_records(epi.buf, idx->ws_fdot.as<double>(), epi.cnt, cap, B, kprime, idx->row_base, idx->d_norm_b, idx->d_created,
                                          idx->d_row_ids, io.kw, io.d_cand, s));
    } else {
        const int32_t group = orr::finish_survivors_group(B, D);
        const int32_t lists_room = std::max<int32_t>(buf_lists, group ? (int32_t)(cap / (uint32_t)group) : 0);
        ORR_TRY(idx->ws_sel.reserve(sizeof(orr::SelEntry) * (size_t)B * (size_t)lists_room * orr::kSelWidth));
        // (the four-launch tail behind rescore_buffer_exact reports no bytes, as behind a screen)
        ORR_TRY(two_stage_tail(idx, a, kprime, idx->n_rows, io, epi, cap, buf_lists, true, f.rec_bytes, how,
                               how == Rescore::BufferExact ? 0.0 : pair_bytes, s));
        HIP_TRY(orr::launch_scope_trailers(io.d_cand, B, kprime, epi.cnt, s));
    }
    ORR_TRY(records_to_host(idx, f, s));
    idx->sstats.pass_mode = 4;
    const int r = finish_pass(idx, a, p, kws, f.n_terms_total);
    if (r != ORR_OK) return r;
    *recs_host = idx->pin_cand.as<orr_candidate>();
    return ORR_OK;
}

// The slices of a scoped call: queries [b0, b0 + nq) whose bitmaps are built together.  A query whose scope brings more rows
// than a pass takes (scope::kMaxScopeRows) is refused before any pass runs.
int32_t scope_slice_width(const orr_index *idx, int32_t B) { return scope::bitmap_slice(B, idx->n_rows, escalation::kPassWorkspaceBytes / 4); }

int open_scope_slice(orr_index *idx, const ScopeArgs &sc, const std::vector<int64_t> &limit, int32_t b0, int32_t per, const char *fn, ScopeSlice &sl)
{
    ORR_TRY(build_scope_slice(idx, sc, limit, b0, std::min<int32_t>(per, (int32_t)limit.size() - b0), sl));
    for (int32_t i = 0; i < sl.nq; ++i)
        if (sl.took[i] > scope::kMaxScopeRows)
            return fail(ORR_EINVAL, "%s: the scope of query %d resolves to %u rows; at most %u scoped rows per query take part in one search "
                        "(lower candidate_limit, or search unscoped)", fn, sl.b0 + i, sl.took[i], scope::kMaxScopeRows);
    return ORR_OK;
}

// One part of a slice after its scoped pass: what the host finish needs of it.
struct ScopedPart {
    std::vector<uint32_t> qsel;         // its queries in the slice's numbering
    std::vector<int32_t> ids;           // ... in the call's
    int32_t kprime = 0;                 // records per query of the pass
    SubBatch sb;
    BatchArgs cur;                      // the part as a batch
    const float *q_host = nullptr;
    const orr_candidate *recs = nullptr;   // [ids.size()][kprime + 1], host memory, valid until the lane's next pass
};

// The queries `q` of a slice through one scoped pass of the form, in parts whose pairs stay within the workspace; done(part)
// after each.  Selection: kprime records per query.  AllRecords: as many as the part's largest scope holds, at least kprime.
template <class Done>
int for_each_scoped_part(orr_index *idx, const BatchArgs &orig, const ScopeSlice &sl, const std::vector<uint32_t> &q, scope::Form form,
                         int32_t kprime, Done &&done)
{
    const bool all = form == scope::Form::AllRecords;
    std::vector<uint32_t> counts(q.size());
    for (size_t i = 0; i < q.size(); ++i) counts[i] = sl.took[q[i]];
    // bytes per pair of a Selection pass on this lane: the smallest group the tail's one-launch form may sort (a sub-batch of one
    // query), where that form runs at all; the records of AllRecords also cross to the host in one piece
    const bool fused_tail = orig.dim > 0 && orig.dim == idx->dim && idx->dim % 256 == 0;
    const size_t pair_bytes = all ? scope::kPairBytesAllRecords : scope::pair_bytes_selection(fused_tail ? orr::finish_survivors_group(1, idx->dim) : 0);
    for (const auto &part : scope::slice_by_pairs(counts, pair_bytes, escalation::kPassWorkspaceBytes / (all ? 4 : 1))) {
        ScopedPart pt;
        pt.qsel.assign(q.begin() + part.first, q.begin() + part.second);
        uint32_t worst = (uint32_t)kprime;
        for (uint32_t i : pt.qsel) { pt.ids.push_back(sl.b0 + (int32_t)i); worst = std::max(worst, sl.took[i]); }
        pt.kprime = all ? (int32_t)worst : kprime;
        ORR_TRY(build_subset(idx, orig, pt.ids, pt.sb, pt.cur));
        ORR_TRY(retry_pass(idx, [&] { return run_scoped_pass(idx, pt.cur, pt.qsel, sl, form, pt.kprime, &pt.q_host, &pt.recs); }));
        idx->sstats.passes += 1;
        ORR_TRY(done(pt));
    }
    return ORR_OK;
}

// orr_search_batch_scoped on the lane the caller holds.
int scoped_batch(orr_index *idx, const BatchArgs &orig, const ScopeArgs &sc, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t B = orig.B, take = std::max<int32_t>(1, orig.topk);
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    for (size_t i = 0; i < (size_t)B * take; ++i) { out_rows[i] = -1; out_scores[i] = 0.0; }
    if (out_counts) for (int32_t b = 0; b < B; ++b) out_counts[b] = 0;
    if (idx->n_rows <= 0 || sc.n_ids == 0) return ORR_OK;
    ORR_TRY(bind_device(idx));
    ORR_TRY(ensure_scope_table(idx));
    const std::vector<int64_t> limit((size_t)B, std::max<int64_t>(1, orig.candidate_limit));     // Take(Math.Max(1, maxCount)), over the scoped rows
    const int32_t per = scope_slice_width(idx, B);
    for (int32_t b0 = 0; b0 < B; b0 += per) {
        ScopeSlice sl;
        ORR_TRY(open_scope_slice(idx, sc, limit, b0, per, "orr_search_batch_scoped", sl));
        struct Todo { std::vector<uint32_t> q; scope::Rung rung; int repeats; };     // queries of the slice and the pass they take next
        Todo first{{}, {}, 0};
        uint32_t max_scope = 0;
        for (int32_t i = 0; i < sl.nq; ++i)
            if (sl.took[i] > 0) { first.q.push_back((uint32_t)i); max_scope = std::max(max_scope, sl.took[i]); }
        if (first.q.empty()) continue;
        first.rung = scope::first_rung(take, max_scope, orr::kSelWidth);
        std::deque<Todo> todo(1, std::move(first));
        while (!todo.empty()) {
            const Todo r = std::move(todo.front());
            todo.pop_front();
            const bool all = r.rung.form == scope::Form::AllRecords;
            Todo next{{}, {}, r.repeats + 1};
            uint32_t next_scope = 0;
            ORR_TRY(for_each_scoped_part(idx, orig, sl, r.q, r.rung.form, all ? 1 : (int32_t)r.rung.kprime, [&](const ScopedPart &pt) -> int {
                std::vector<uint8_t> cert;
                ORR_TRY(merge_into(1, pt.kprime, pt.recs, pt.cur, use_cos, pt.q_host, idx->h_norm_a.data(), pt.ids, out_rows, out_scores, out_counts, cert));
                for (size_t i = 0; i < cert.size(); ++i)
                    if (!cert[i]) { next.q.push_back(pt.qsel[i]); next_scope = std::max(next_scope, sl.took[pt.qsel[i]]); }
                if (r.repeats > 0) idx->sstats.requeried += (int64_t)pt.ids.size();
                return ORR_OK;
            }));
            if (next.q.empty()) continue;
            next.rung = scope::next_rung(r.rung, next_scope, orr::kSelWidth);
            if (next.rung.form == scope::Form::Done || next.repeats > scope::kMaxRungs)
                return fail(ORR_EDEVICE, "orr_search_batch_scoped: a pass over every scoped row left a query uncertified");
            todo.push_front(std::move(next));
        }
    }
    return ORR_OK;
}

// ---- masked search: one scope shared by every query of the batch, screened once per batch (orr_search_batch_masked) ---------
// The scope resolves to ONE bitmap as a shared scoped list does; then, instead of re-scoring every listed row per query, the
// two-stage screen of the unscoped pass runs over rows [0, n_clip) with the mask in its row constants, a filter behind it makes
// the mask exact, and the exact tail ranks what is left.  Large scopes that the cost rule leaves to the list path, ineligible
// passes and the end of the ladder run the scoped pass over the bitmap in parts.  The rules are orr_mask_plan.h's.

// Where the ONE scope of a masked call comes from: a list of ids, resolved by the call, or a scope handle (the caller holds it
// shared and has checked that it belongs to this shard).
struct ScopeSource {
    const ScopeArgs *list = nullptr;
    const orr_scope *handle = nullptr;
    bool empty() const { return handle ? handle->live.load() <= 0 : list->n_ids == 0; }
};

constexpr int kNotMaskable = 2;        // run_masked_pass: plan_form found no two-stage form for the batch (k' beyond a list, no shadow): the list path

// One masked pass over the queries of `a`: run_shard_once's front end and stages over rows [0, ms.n_clip), no prefix (the floor
// comes from an in-scope sample, masked_floor), the survivors filtered by the mask in front of the tail.  Records in host
// memory (*recs_host).  kRetryPass as run_shard_once; kNotMaskable before anything ran.  Caller holds the lane and its lock.
// With `groups` the pass is a grouped one (orr_search_batch_masked_groups): ms carries the largest clip and the largest sample, the
// row constants, the sample, the filter and the trailers take each query's own group from `groups`.
int run_masked_pass(orr_index *idx, const BatchArgs &a, int32_t kprime, const MaskScope &ms, const float **q_host,
                    const orr_candidate **recs_host, PassPlan &p, GroupScopes *groups = nullptr)
{
    ORR_TRY(bind_device(idx));
    const int64_t n = ms.n_clip;
    const int32_t B = a.B;
    hipStream_t s = idx->stream;
    *recs_host = nullptr;
    PassFront f;
    auto plan = [&](const std::vector<uint32_t> &qoff, PassPlan &pl) -> int {
        ORR_TRY(plan_pass(idx, a, kprime, n, qoff, pl));
        if (!pl.two_stage()) return kNotMaskable;
        pl.masked = true;
        pl.grouped = groups != nullptr;
        pl.rowc_inline = false;        // the mask lives in the materialised row constants: the int8 stream reads them too
        return ORR_OK;
    };
    ORR_TRY(open_pass(idx, a, kprime, plan, true, false, false, q_host, p, f));
    PassIo &io = f.io;
    io.mask = &ms;
    io.groups = groups;
    if (p.screen == Screen::GemvI8) ORR_TRY(launch_i8_query_image(idx, io.d_q, B, false, s));
    KwSide kws;
    ORR_TRY(launch_keyword_side(idx, a, f.qoff, kws));
    io.kw = kws.view;
    ORR_TRY(launch_numerators(idx, a, p, n, io));
    ORR_TRY(launch_consts(idx, a, p, n, f.qoff, f.q_download_pending, io));
    if (f.n_terms_total > 0) HIP_TRY(hipStreamWaitEvent(s, idx->ev_kw_done, 0));
    ORR_TRY(launch_selection(idx, a, p, kprime, n, io, true, f.rec_bytes));
    // (no record of a deleted row: the mask never held one)
    ORR_TRY(records_to_host(idx, f, s));
    idx->sstats.pass_mode = p.pass_mode();
    const int r = finish_pass(idx, a, p, kws, f.n_terms_total);
    if (r != ORR_OK) return r;
    if (groups && groups->h_screened && idx->profiling == 1) {
        // "grouped_screen_pairs": 16 bytes per pair the screen buffered in front of the filter (what mask_survivors_grouped read)
        double pairs = 0.0;
        for (int32_t b = 0; b < B; ++b) pairs += (double)std::min<uint32_t>(groups->h_screened[b], idx->pass_cap);
        add_phase_stat(idx, "grouped_screen_pairs", std::chrono::steady_clock::now(), 16.0 * pairs);
    }
    *recs_host = io.direct_host ? io.d_cand : idx->pin_cand.as<orr_candidate>();
    return ORR_OK;
}

// One rung of the list path for the queries `gids` of the call (ascending): the scope's first ms.took rows cut by rank into P
// parts of at most mask_part_rows, each part a scoped pass of `form` over every query (for_each_scoped_part); the parts' records
// in store [P][gids.size()][K + 1] as shards' records are laid out, the queries' exact norms in norms.  K: k' of a Selection
// pass, the largest part of an AllRecords one.  `sl` is the call's slice (b0 = 0, every query of the call, one shared bitmap
// in ws_scope_bm, which a part overwrites when there are several).
int list_part_records(orr_index *idx, const BatchArgs &orig, const ScopeSlice &call_sl, const MaskScope &ms, const std::vector<int32_t> &gids,
                      scope::Form form, int64_t K, bool requery, std::vector<orr_candidate> &store, std::vector<double> &norms)
{
    ScopeSlice sl = call_sl;
    const bool all = form == scope::Form::AllRecords;
    const int64_t part_rows = idx->opt_mask_part_rows;
    const int64_t P = mask::part_count(ms.took, part_rows);
    hipStream_t s = idx->stream;
    uint32_t *h_live = const_cast<uint32_t *>(sl.live), *h_took = const_cast<uint32_t *>(sl.took);       // pin_scope: a part's counts land there
    const size_t nb = gids.size(), rec_q = (size_t)K + 1;
    const std::vector<uint32_t> q(gids.begin(), gids.end());                  // the slice's numbering is the call's
    store.assign((size_t)P * nb * rec_q, orr_candidate{});
    norms.assign(nb, 0.0);
    if (P > 1) {           // the parts are written into the lane's own workspace, whoever owns the scope's bitmap
        ORR_TRY(idx->ws_scope_bm.reserve(sizeof(uint32_t) * (size_t)sl.words));
        ORR_TRY(idx->ws_scope_chunks.reserve(sizeof(uint32_t) * (size_t)orr::scope_chunks(sl.words)));
        sl.bm = idx->ws_scope_bm.as<uint32_t>(); sl.chunks = idx->ws_scope_chunks.as<uint32_t>();
    }
    for (int64_t j = 0; j < P; ++j) {
        if (P > 1) {       // this part's bitmap and counts; candidate_limit is already in the clip to ms.took
            const auto range = mask::part_range(j, ms.took, part_rows);
            Timed t(idx, "mask_part", 8.0 * (double)ms.words);
            HIP_TRY(orr::launch_mask_part(ms.bm, ms.words, ms.chunks, (uint64_t)range.first, (uint64_t)range.second,
                                          idx->ws_scope_bm.as<uint32_t>(), s));
            HIP_TRY(orr::launch_scope_counts(idx->ws_scope_bm.as<uint32_t>(), sl.words, 1, sl.nq, sl.d_limit,
                                             idx->ws_scope_chunks.as<uint32_t>(), h_live, h_took, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        collect_events(idx);
        ORR_TRY(for_each_scoped_part(idx, orig, sl, q, form, all ? 1 : (int32_t)K, [&](const ScopedPart &pt) -> int {
            for (size_t i = 0; i < pt.ids.size(); ++i) {
                const size_t at = (size_t)(std::lower_bound(gids.begin(), gids.end(), pt.ids[i]) - gids.begin());
                orr_candidate *dst = store.data() + ((size_t)j * nb + at) * rec_q;
                const orr_candidate *src = pt.recs + i * ((size_t)pt.kprime + 1);
                const size_t have = std::min<size_t>((size_t)pt.kprime, (size_t)K);
                memcpy(dst, src, sizeof(orr_candidate) * have);
                for (size_t e = have; e < (size_t)K; ++e) { memset(&dst[e], 0, sizeof(dst[e])); dst[e].row_id = -1; dst[e].order_key = -1; }
                dst[K] = src[pt.kprime];
                norms[at] = idx->h_norm_a[i];
            }
            if (requery && j == 0) idx->sstats.requeried += (int64_t)pt.ids.size();
            return ORR_OK;
        }));
    }
    return ORR_OK;
}

// The list path in parts for the queries `ids` of the call (ascending): the scope's first ms.took rows cut by rank into parts
// of at most mask_part_rows, each part a scoped pass over every query (for_each_scoped_part), the parts' records merged per
// query as shards in global order are; an uncertified query climbs scope::next_rung over all parts.  `sl` is the call's slice
// (b0 = 0, every query of the call, one shared bitmap in ws_scope_bm, which a part overwrites when there are several).
int masked_list_path(orr_index *idx, const BatchArgs &orig, const ScopeSlice &sl, const MaskScope &ms, const std::vector<int32_t> &ids,
                     bool requery, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t take = std::max<int32_t>(1, orig.topk);
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    const int64_t part_rows = idx->opt_mask_part_rows;
    const int64_t P = mask::part_count(ms.took, part_rows);
    if (P > (1 << 16)) return fail(ORR_EINVAL, "orr_search_batch_masked: mask_part_rows %lld cuts the scope into %lld parts", (long long)part_rows, (long long)P);
    const int64_t max_part = std::min<int64_t>(ms.took, part_rows);
    struct Todo { std::vector<int32_t> ids; scope::Rung rung; int repeats; };
    std::deque<Todo> todo(1, Todo{ids, scope::first_rung(take, max_part, orr::kSelWidth), requery ? 1 : 0});
    while (!todo.empty()) {
        const Todo r = std::move(todo.front());
        todo.pop_front();
        const bool all = r.rung.form == scope::Form::AllRecords;
        const int64_t K = all ? std::max<int64_t>(1, max_part) : r.rung.kprime;       // records per query and part
        const int32_t n_ids = (int32_t)r.ids.size();
        const int32_t group = mask::merge_group(n_ids, P, K, mask::kMergeBudgetBytes);
        Todo next{{}, {}, r.repeats + 1};
        for (int32_t g0 = 0; g0 < n_ids; g0 += group) {
            const std::vector<int32_t> gids(r.ids.begin() + g0, r.ids.begin() + std::min<int32_t>(n_ids, g0 + group));
            std::vector<orr_candidate> store;
            std::vector<double> norms;
            ORR_TRY(list_part_records(idx, orig, sl, ms, gids, r.rung.form, K, r.repeats > 0, store, norms));
            SubBatch sb;
            BatchArgs cur;
            ORR_TRY(build_subset(idx, orig, gids, sb, cur));
            std::vector<uint8_t> cert;
            ORR_TRY(merge_into((int32_t)P, (int32_t)K, store.data(), cur, use_cos, nullptr, norms.data(), gids, out_rows, out_scores, out_counts, cert));
            for (size_t i = 0; i < cert.size(); ++i)
                if (!cert[i]) next.ids.push_back(gids[i]);
        }
        if (next.ids.empty()) continue;
        next.rung = scope::next_rung(r.rung, max_part, orr::kSelWidth);
        if (next.rung.form == scope::Form::Done || next.repeats > scope::kMaxRungs + 1)
            return fail(ORR_EDEVICE, "orr_search_batch_masked: a pass over every scoped row left a query uncertified");
        todo.push_front(std::move(next));
    }
    return ORR_OK;
}

// The queries `ids` of the call through the masked screen and its ladder (mask::next_step).  The ladder is a query's: of the
// queries a pass leaves uncertified, those whose overflowing buffer can be grown repeat together, the others take the next rung.
int masked_screen_ladder(orr_index *idx, const BatchArgs &orig, const ScopeSlice &sl, const MaskScope &ms, std::vector<int32_t> first_ids,
                         int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t take = std::max<int32_t>(1, orig.topk);
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    struct Todo { std::vector<int32_t> ids; int64_t kprime; bool grown; int repeats; };
    std::deque<Todo> todo(1, Todo{std::move(first_ids), escalation::initial_kprime(take, ms.took, orr::kSelWidth), false, 0});
    while (!todo.empty()) {
        const Todo r = std::move(todo.front());
        todo.pop_front();
        const size_t nb = r.ids.size();
        SubBatch sb;
        BatchArgs cur;
        ORR_TRY(build_subset(idx, orig, r.ids, sb, cur));
        PassPlan pass;
        const float *q_host = nullptr;
        const orr_candidate *recs = nullptr;
        const int rc = retry_pass(idx, [&] { return run_masked_pass(idx, cur, (int32_t)r.kprime, ms, &q_host, &recs, pass); });
        if (rc == kNotMaskable) {
            ORR_TRY(masked_list_path(idx, orig, sl, ms, r.ids, r.repeats > 0, out_rows, out_scores, out_counts));
            continue;
        }
        if (rc != ORR_OK) return rc;
        std::vector<uint8_t> cert;
        ORR_TRY(merge_into(1, (int32_t)r.kprime, recs, cur, use_cos, q_host, idx->h_norm_a.data(), r.ids, out_rows, out_scores, out_counts, cert));
        const ShardOutcome o = outcome_of(idx, pass, ms.n_clip);
        idx->sstats.passes += 1;
        if (r.repeats > 0) idx->sstats.requeried += (int64_t)nb;
        escalation::account_survivors(idx->sstats, o, nb);
        size_t n_again = 0;
        for (size_t i = 0; i < nb; ++i) n_again += cert[i] ? 0 : 1;
        if (n_again == 0) continue;
        // uncertified queries: those that overflowed a buffer larger ones can hold, and the rest
        std::vector<int32_t> grow, rest;
        uint32_t worst = 0, cap_i = 0;
        for (size_t i = 0; i < nb; ++i) {
            if (cert[i]) continue;
            if (!r.grown && o.kept(nb) && o.overflowed(i) && escalation::grown_survivor_cap(o.pass_cap, o.survivors[i], ms.n_clip, n_again, &cap_i)) {
                grow.push_back(r.ids[i]);
                worst = std::max(worst, o.survivors[i]);
            } else {
                rest.push_back(r.ids[i]);
            }
        }
        if (r.repeats >= mask::kMaxScreenRepeats) { rest.insert(rest.end(), grow.begin(), grow.end()); std::sort(rest.begin(), rest.end()); grow.clear(); }
        if (!rest.empty()) {
            const mask::Next nx = mask::next_step(false, r.grown, o.pass_cap, 0, ms.n_clip, rest.size(), r.kprime, orr::kSelWidth);
            if (nx.step == mask::Step::WiderK && r.repeats < mask::kMaxScreenRepeats) todo.push_back(Todo{rest, nx.kprime, r.grown, r.repeats + 1});
            else ORR_TRY(masked_list_path(idx, orig, sl, ms, rest, true, out_rows, out_scores, out_counts));
        }
        if (!grow.empty()) {
            const mask::Next nx = mask::next_step(true, r.grown, o.pass_cap, worst, ms.n_clip, grow.size(), r.kprime, orr::kSelWidth);
            if (nx.step != mask::Step::GrowBuffers) {
                ORR_TRY(masked_list_path(idx, orig, sl, ms, grow, true, out_rows, out_scores, out_counts));
                continue;
            }
            idx->sstats.buffer_growths += 1;       // the index keeps the larger size, as for the unscoped search
            if (nx.new_cap > idx->survivor_cap) idx->survivor_cap = nx.new_cap;
            if (!idx->is_view || idx->internal_lane) publish_survivor_hint(const_cast<orr_index *>(owner_of(idx)), nx.new_cap);
            todo.push_back(Todo{grow, nx.kprime, true, r.repeats + 1});
        }
    }
    return ORR_OK;
}

// The ONE scope of a masked call on the lane the caller holds (the id table exists): resolved to a shared bitmap whose first
// `limit` live rows take part, kept beside the slice's (which the list path rewrites per part), clipped, the sample sized for
// the caller's k.  ms.took == 0: nothing takes part, and nothing but words / live / took is set.
// The source is a list of ids, resolved now, or a scope handle, which holds all of it already: then no id goes up, no lookup and
// no count runs, the bitmap is read where it lies, and a call whose limit reaches every row of the scope takes the handle's
// n_clip_all without a launch or a synchronise.
int resolve_mask_scope(orr_index *idx, int32_t B, int32_t topk, const ScopeSource &src, int64_t limit_rows, ScopeSlice &sl, MaskScope &ms)
{
    hipStream_t s = idx->stream;
    if (src.handle) {
        const orr_scope *h = src.handle;
        ORR_TRY(slice_of_handle(idx, h, B, limit_rows, sl));
        ms.words = sl.words; ms.live = sl.live[0]; ms.took = sl.took[0];
        if (ms.took == 0) return ORR_OK;
        ms.bm = h->bm; ms.chunks = h->chunks;
        ms.n_clip = h->n_clip_all;
        if (ms.took < ms.live) {
            ORR_TRY(idx->pin_mask.reserve(sizeof(int64_t)));
            {
                Timed t(idx, "mask_clip", 4.0 * (double)orr::kScopeChunkWords + 4.0 * (double)orr::scope_chunks(ms.words));
                HIP_TRY(orr::launch_mask_clip(ms.bm, ms.words, ms.chunks, (uint32_t)ms.took, idx->pin_mask.as<int64_t>(), s));
            }
            HIP_TRY(hipStreamSynchronize(s));
            collect_events(idx);
            ms.n_clip = std::min<int64_t>(*idx->pin_mask.as<int64_t>(), idx->n_rows);
        }
        ms.sample = mask::sample_rows(topk, ms.took);
        return ORR_OK;
    }
    // ---- resolve: one shared bitmap; live and took are the same for every query
    const std::vector<int64_t> limit((size_t)B, limit_rows);
    ORR_TRY(build_scope_slice(idx, *src.list, limit, 0, B, sl));
    ms.words = sl.words; ms.live = sl.live[0]; ms.took = sl.took[0];
    if (ms.took == 0) return ORR_OK;
    // ---- the scope's bitmap is kept beside the slice's; clip
    const size_t bm_bytes = sizeof(uint32_t) * (size_t)ms.words, ch_bytes = sizeof(uint32_t) * (size_t)orr::scope_chunks(ms.words);
    ORR_TRY(idx->ws_mask_bm.reserve(bm_bytes));
    ORR_TRY(idx->ws_mask_chunks.reserve(ch_bytes));
    ORR_TRY(idx->pin_mask.reserve(sizeof(int64_t)));
    HIP_TRY(hipMemcpyAsync(idx->ws_mask_bm.p, idx->ws_scope_bm.p, bm_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(idx->ws_mask_chunks.p, idx->ws_scope_chunks.p, ch_bytes, hipMemcpyDeviceToDevice, s));
    ms.bm = idx->ws_mask_bm.as<uint32_t>(); ms.chunks = idx->ws_mask_chunks.as<uint32_t>();
    {
        Timed t(idx, "mask_clip", 4.0 * (double)orr::kScopeChunkWords + (double)ch_bytes);
        HIP_TRY(orr::launch_mask_clip(ms.bm, ms.words, ms.chunks, (uint32_t)ms.took, idx->pin_mask.as<int64_t>(), s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(idx);
    ms.n_clip = std::min<int64_t>(*idx->pin_mask.as<int64_t>(), idx->n_rows);
    ms.sample = mask::sample_rows(topk, ms.took);
    return ORR_OK;
}

// orr_search_batch_masked on the lane the caller holds.
int masked_batch(orr_index *idx, const BatchArgs &orig, const ScopeSource &src, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t B = orig.B, take = std::max<int32_t>(1, orig.topk);
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    for (size_t i = 0; i < (size_t)B * take; ++i) { out_rows[i] = -1; out_scores[i] = 0.0; }
    if (out_counts) for (int32_t b = 0; b < B; ++b) out_counts[b] = 0;
    if (idx->n_rows <= 0 || src.empty()) return ORR_OK;
    ORR_TRY(bind_device(idx));
    if (src.list) ORR_TRY(ensure_scope_table(idx));
    ScopeSlice sl;
    MaskScope ms;
    ORR_TRY(resolve_mask_scope(idx, B, orig.topk, src, std::max<int64_t>(1, orig.candidate_limit), sl, ms));
    if (ms.took == 0) return ORR_OK;
    // ---- the screen or the list path
    const bool eligible = mask::eligible(use_cos, idx->dim, orig.topk, orr::kSelWidth, ms.n_clip, idx->opt_two_stage, ms.took);
    std::vector<int32_t> ids((size_t)B);
    std::iota(ids.begin(), ids.end(), 0);
    if (mask::choose(idx->opt_mask_screen, eligible, B, ms.took, ms.n_clip) == mask::Path::List)
        return masked_list_path(idx, orig, sl, ms, ids, false, out_rows, out_scores, out_counts);
    const int32_t per = mask::screen_slice(B, ms.sample);
    for (int32_t b0 = 0; b0 < B; b0 += per)
        ORR_TRY(masked_screen_ladder(idx, orig, sl, ms, std::vector<int32_t>(ids.begin() + b0, ids.begin() + std::min<int32_t>(B, b0 + per)),
                                     out_rows, out_scores, out_counts));
    return ORR_OK;
}

// ---- grouped masked search: G scopes, each shared by the queries that name it, screened together (orr_search_batch_masked_groups)
// Each group alone is a masked search; what the groups share is the one stream over the shard's shadow.  The rules -- which
// groups screen together, their samples, the cost rule, the ladder -- are orr_group_plan.h's.

struct GroupArgs {
    int32_t n_groups;
    int64_t n_ids;
    const int64_t *ids;            // host or device
    const uint64_t *off;           // host [n_groups + 1]
    const int32_t *query_group;    // host [B]
    const orr_scope *const *scopes = nullptr;   // [n_groups] instead of the lists (orr_search_batch_in_scopes): held shared by the caller
    bool listed(int32_t g) const { return scopes ? scopes[g]->live.load() > 0 : off[g + 1] > off[g]; }
};

// The queries `ids` of the call (ascending, all of group g) as a masked call of their own, the results scattered back.
int masked_sub_batch(orr_index *idx, const BatchArgs &orig, const GroupArgs &ga, int32_t g, const std::vector<int32_t> &ids,
                     int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    if (ids.empty()) return ORR_OK;
    const int32_t take = std::max<int32_t>(1, orig.topk);
    ScopeArgs sc{0, nullptr, nullptr, nullptr};
    if (!ga.scopes) sc = ScopeArgs{(int64_t)(ga.off[g + 1] - ga.off[g]), ga.ids ? ga.ids + ga.off[g] : nullptr, nullptr, nullptr};
    const ScopeSource src{ga.scopes ? nullptr : &sc, ga.scopes ? ga.scopes[g] : nullptr};
    SubBatch sb;
    BatchArgs cur;
    ORR_TRY(build_subset(idx, orig, ids, sb, cur));
    if (cur.B == orig.B) return masked_batch(idx, cur, src, out_rows, out_scores, out_counts);      // every query of the call
    const size_t nb = ids.size();
    std::vector<int64_t> rows(nb * (size_t)take);
    std::vector<double> scores(nb * (size_t)take);
    std::vector<int32_t> counts(nb);
    std::vector<int64_t> keys(orig.out_keys ? nb * (size_t)take : 0);      // (out_keys is in the numbering of the call that receives it)
    if (orig.out_keys) cur.out_keys = keys.data();
    ORR_TRY(masked_batch(idx, cur, src, rows.data(), scores.data(), counts.data()));
    for (size_t i = 0; i < nb; ++i) {
        const size_t b = (size_t)ids[i];
        if (orig.out_keys) memcpy(orig.out_keys + b * take, keys.data() + i * take, sizeof(int64_t) * take);
        memcpy(out_rows + b * take, rows.data() + i * take, sizeof(int64_t) * take);
        memcpy(out_scores + b * take, scores.data() + i * take, sizeof(double) * take);
        if (out_counts) out_counts[b] = counts[i];
    }
    return ORR_OK;
}

// `ids` (ascending) split by group, each part a masked call of its own.  The call resolves its group again instead of taking
// the bitmap the grouped resolve holds: masked_screen_ladder ends in masked_list_path, which reads ONE shared bitmap with its
// pinned counts and device limits from the lane's scoped slice (ws_scope_bm, pin_scope, ws_scope_meta) and rewrites it per
// part -- the grouped resolve left G bitmaps and G pseudo-queries there, and a slice rebuilt by hand from them would be a
// second copy of build_scope_slice's layout.  One scope_lookup of the group's ids (14-55 us measured) on a path that runs only
// for queries the grouped pass could not certify buys that the ladder is the masked call's, unchanged and already tested.
int masked_sub_batches(orr_index *idx, const BatchArgs &orig, const GroupArgs &ga, const std::vector<int32_t> &ids, bool requery,
                       int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    std::vector<std::vector<int32_t>> by_group((size_t)ga.n_groups);
    for (int32_t b : ids) by_group[(size_t)ga.query_group[b]].push_back(b);
    for (int32_t g = 0; g < ga.n_groups; ++g) {
        if (by_group[(size_t)g].empty()) continue;
        if (requery) idx->sstats.requeried += (int64_t)by_group[(size_t)g].size();
        ORR_TRY(masked_sub_batch(idx, orig, ga, g, by_group[(size_t)g], out_rows, out_scores, out_counts));
    }
    return ORR_OK;
}

// The queries `first_ids` of the call (all of screen groups) through the grouped pass and its ladder (group::next_step): the
// queries whose only problem was an overflowing buffer repeat together once, with buffers of the call's own; every other
// uncertified query enters its group's masked call.
int grouped_screen_ladder(orr_index *idx, const BatchArgs &orig, const GroupArgs &ga, GroupScopes &gs, const MaskScope &ms,
                          std::vector<int32_t> first_ids, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t take = std::max<int32_t>(1, orig.topk);
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    const int32_t kprime = (int32_t)escalation::initial_kprime(take, ms.took, orr::kSelWidth);
    std::vector<int32_t> ids = std::move(first_ids);
    bool grown = false;
    gs.cap = 0;
    for (int pass_no = 0; !ids.empty(); ++pass_no) {
        const size_t nb = ids.size();
        SubBatch sb;
        BatchArgs cur;
        ORR_TRY(build_subset(idx, orig, ids, sb, cur));
        gs.qgroup.resize(nb);
        for (size_t i = 0; i < nb; ++i) gs.qgroup[i] = ga.query_group[ids[i]];
        PassPlan pass;
        const float *q_host = nullptr;
        const orr_candidate *recs = nullptr;
        const int rc = retry_pass(idx, [&] { return run_masked_pass(idx, cur, kprime, ms, &q_host, &recs, pass, &gs); });
        if (rc == kNotMaskable) return masked_sub_batches(idx, orig, ga, ids, pass_no > 0, out_rows, out_scores, out_counts);
        if (rc != ORR_OK) return rc;
        std::vector<uint8_t> cert;
        ORR_TRY(merge_into(1, kprime, recs, cur, use_cos, q_host, idx->h_norm_a.data(), ids, out_rows, out_scores, out_counts, cert));
        const ShardOutcome o = outcome_of(idx, pass, ms.n_clip);       // (survivor_cap: the lane's, which the call's own growth leaves alone)
        idx->sstats.passes += 1;
        if (pass_no > 0) idx->sstats.requeried += (int64_t)nb;
        escalation::account_survivors(idx->sstats, o, nb);
        size_t n_again = 0;
        for (size_t i = 0; i < nb; ++i) n_again += cert[i] ? 0 : 1;
        if (n_again == 0) break;
        std::vector<int32_t> grow, rest;
        uint32_t worst = 0, cap_i = 0;
        for (size_t i = 0; i < nb; ++i) {
            if (cert[i]) continue;
            if (!grown && pass_no + 1 < group::kMaxGroupedPasses && o.kept(nb) && o.overflowed(i) &&
                escalation::grown_survivor_cap(o.pass_cap, o.survivors[i], ms.n_clip, n_again, &cap_i)) {
                grow.push_back(ids[i]);
                worst = std::max(worst, o.survivors[i]);
            } else {
                rest.push_back(ids[i]);
            }
        }
        group::Next nx;
        if (!grow.empty()) nx = group::next_step(true, grown, o.pass_cap, worst, ms.n_clip, grow.size());
        if (nx.step != group::Step::GrowBuffers) { rest.insert(rest.end(), grow.begin(), grow.end()); std::sort(rest.begin(), rest.end()); grow.clear(); }
        ORR_TRY(masked_sub_batches(idx, orig, ga, rest, true, out_rows, out_scores, out_counts));
        if (grow.empty()) break;
        idx->sstats.buffer_growths += 1;       // the call's own: neither the lane nor the handle keeps the size
        gs.cap = nx.new_cap;
        grown = true;
        ids = std::move(grow);
    }
    gs.cap = 0;
    return ORR_OK;
}

// The front of a grouped call on the lane the caller holds: resolve (G bitmaps; the handles bring theirs), gather, clip, plan.
// took: with handles, the rows of each group that take part on this shard (the caller's rule: the index call's
// group::took_of, the shard form's cscope::shard_took); ignored for lists, whose slice counts them under the call's limit.
struct GroupFront {
    ScopeSlice sl;
    std::vector<group::GroupIn> gin;
    int32_t n_used = 0, only = -1;      // n_used <= 1: nothing below is set -- no group, or the masked call of group `only`
    group::Plan plan;
    GroupScopes gs;
    MaskScope ms;                       // the scopes as a whole: what the stages ask of one (set with `screened`)
    std::vector<int32_t> screened;      // ascending: the queries of the grouped pass (empty: it does not run)
};

int grouped_front(orr_index *idx, const BatchArgs &call, const GroupArgs &ga, const std::vector<std::vector<int32_t>> &members,
                  const int64_t *took, GroupFront &f)
{
    const int32_t B = call.B, G = ga.n_groups;
    const bool use_cos = call.dim > 0 && call.dim == idx->dim;
    hipStream_t s = idx->stream;
    // ---- resolve: the groups as G pseudo-queries of a scoped slice -> G bitmaps, live and took per group; handles bring theirs
    const std::vector<int64_t> limit((size_t)G, std::max<int64_t>(1, call.candidate_limit));
    const ScopeArgs sc{ga.n_ids, ga.ids, ga.off, nullptr};
    ScopeSlice &sl = f.sl;
    std::vector<group::GroupIn> &gin = f.gin;
    gin.assign((size_t)G, group::GroupIn{});
    if (ga.scopes) {
        sl.words = ga.scopes[0]->words;
        for (int32_t g = 0; g < G; ++g) gin[(size_t)g].took = took[g];
    } else {
        ORR_TRY(ensure_scope_table(idx));
        ORR_TRY(build_scope_slice(idx, sc, limit, 0, G, sl));
        for (int32_t g = 0; g < G; ++g) gin[(size_t)g].took = sl.took[g];
    }
    for (int32_t g = 0; g < G; ++g) gin[(size_t)g].queries = (int32_t)members[(size_t)g].size();
    f.n_used = 0; f.only = -1;
    for (int32_t g = 0; g < G; ++g)
        if (group::used(gin[(size_t)g])) { f.n_used += 1; f.only = g; }
    if (f.n_used <= 1) return ORR_OK;
    // ---- the bitmaps are kept beside the slice's (which a group's own masked call rewrites); clip per used group
    GroupScopes &gs = f.gs;
    gs.n_groups = G; gs.words = sl.words;
    const int32_t n_chunks = orr::scope_chunks(sl.words);
    const size_t bm_bytes = sizeof(uint32_t) * (size_t)G * (size_t)sl.words, ch_bytes = sizeof(uint32_t) * (size_t)G * (size_t)n_chunks;
    ORR_TRY(idx->ws_group_bm.reserve(bm_bytes));
    ORR_TRY(idx->ws_group_chunks.reserve(ch_bytes));
    ORR_TRY(idx->pin_group.reserve(sizeof(int64_t) * 2 * (size_t)G + sizeof(uint32_t) * (size_t)B));      // [clip x G][sample x G][screened x B]
    ORR_TRY(idx->ws_group_meta.reserve(sizeof(int64_t) * 2 * (size_t)G));
    gs.bm = idx->ws_group_bm.as<uint32_t>(); gs.chunks = idx->ws_group_chunks.as<uint32_t>();
    int64_t *h_meta = idx->pin_group.as<int64_t>();            // [clip x G][sample x G]
    for (int32_t g = 0; g < 2 * G; ++g) h_meta[g] = 0;
    bool clipped = false;
    if (ga.scopes) {
        // the used handles' arrays, gathered (the grouped stages want them contiguous; an unused group's are never read), and the
        // clip of every handle not all of whose rows take part: one launch
        orr::GroupGatherTable tab{};
        int32_t n_entries = 0;
        for (int32_t g = 0; g < G; ++g) {
            if (!group::used(gin[(size_t)g])) continue;
            if (ga.scopes[g]->words != sl.words) return fail(ORR_ESTATE, "grouped search: the scopes cover different numbers of rows");
            const bool clip = gin[(size_t)g].took < ga.scopes[g]->live.load();
            tab.bm[n_entries] = ga.scopes[g]->bm; tab.chunks[n_entries] = ga.scopes[g]->chunks;
            tab.clip_took[n_entries] = clip ? (uint32_t)gin[(size_t)g].took : 0u;
            tab.slot[n_entries] = g;
            n_entries += 1;
            clipped = clipped || clip;
        }
        {
            Timed t(idx, "group_gather_clip", 2.0 * 4.0 * ((double)sl.words + (double)n_chunks) * (double)n_entries);
            HIP_TRY(orr::launch_group_gather_clip(tab, n_entries, G, sl.words, idx->ws_group_bm.as<uint32_t>(), idx->ws_group_chunks.as<uint32_t>(),
                                                  h_meta, s));
        }
    } else {
        HIP_TRY(hipMemcpyAsync(idx->ws_group_bm.p, idx->ws_scope_bm.p, bm_bytes, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(idx->ws_group_chunks.p, idx->ws_scope_chunks.p, ch_bytes, hipMemcpyDeviceToDevice, s));
        for (int32_t g = 0; g < G; ++g) {
            if (!group::used(gin[(size_t)g])) continue;
            Timed t(idx, "mask_clip", 4.0 * (double)orr::kScopeChunkWords + 4.0 * (double)n_chunks);
            HIP_TRY(orr::launch_mask_clip(gs.bm + (size_t)g * (size_t)sl.words, sl.words, gs.chunks + (size_t)g * (size_t)n_chunks,
                                          (uint32_t)gin[(size_t)g].took, h_meta + g, s));
            clipped = true;
        }
    }
    if (clipped || !ga.scopes) {
        HIP_TRY(hipStreamSynchronize(s));
        collect_events(idx);
    }
    for (int32_t g = 0; g < G; ++g) {
        if (ga.scopes && group::used(gin[(size_t)g]) && gin[(size_t)g].took == ga.scopes[g]->live.load()) h_meta[g] = ga.scopes[g]->n_clip_all;
        gin[(size_t)g].n_clip = std::min<int64_t>(h_meta[g], idx->n_rows);
    }
    // ---- the plan: samples, screen and list groups, the grouped pass or a masked call per group
    const uint32_t cap = group::pass_cap(idx->survivor_cap, B);
    f.plan = group::plan(gin, call.topk, cap, idx->opt_mask_screen, use_cos, idx->dim, orr::kSelWidth, idx->opt_two_stage);
    const group::Plan &plan = f.plan;
    f.screened.clear();
    for (int32_t g = 0; g < G; ++g)
        if (plan.grouped && plan.role[(size_t)g] == group::Role::Screen) f.screened.insert(f.screened.end(), members[(size_t)g].begin(), members[(size_t)g].end());
    return ORR_OK;
}

// What the grouped pass over f.screened reads, on the device (after the groups' own calls: they use the lane).
int grouped_front_upload(orr_index *idx, const BatchArgs &call, GroupFront &f)
{
    const int32_t G = f.gs.n_groups;
    const group::Plan &plan = f.plan;
    GroupScopes &gs = f.gs;
    hipStream_t s = idx->stream;
    int64_t *h_meta = idx->pin_group.as<int64_t>();
    std::sort(f.screened.begin(), f.screened.end());
    gs.took.resize((size_t)G); gs.n_clip.resize((size_t)G); gs.sample = plan.sample;
    for (int32_t g = 0; g < G; ++g) {
        gs.took[(size_t)g] = f.gin[(size_t)g].took;
        gs.n_clip[(size_t)g] = f.gin[(size_t)g].n_clip;
        h_meta[g] = group::screen_clip(plan.role[(size_t)g] == group::Role::Screen, f.gin[(size_t)g].n_clip);
        h_meta[G + g] = plan.sample[(size_t)g];
    }
    HIP_TRY(hipMemcpyAsync(idx->ws_group_meta.p, h_meta, sizeof(int64_t) * 2 * (size_t)G, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                      // (pin_group is the next grouped call's on this lane)
    gs.d_clip = idx->ws_group_meta.as<int64_t>(); gs.d_sample = gs.d_clip + G;
    gs.floor_heads = group::floor_from_heads(plan.min_sample, call.topk, orr::kSelWidth);
    gs.h_screened = reinterpret_cast<uint32_t *>(h_meta + 2 * G);
    f.ms = MaskScope{};
    f.ms.words = f.sl.words; f.ms.took = plan.min_took; f.ms.live = plan.min_took;
    f.ms.n_clip = plan.n_clip; f.ms.sample = plan.max_sample;
    return ORR_OK;
}

// orr_search_batch_masked_groups on the lane the caller holds.
int grouped_batch(orr_index *idx, const BatchArgs &call, const GroupArgs &ga, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t B = call.B, take = std::max<int32_t>(1, call.topk), G = ga.n_groups;
    for (size_t i = 0; i < (size_t)B * take; ++i) { out_rows[i] = -1; out_scores[i] = 0.0; }
    if (out_counts) for (int32_t b = 0; b < B; ++b) out_counts[b] = 0;
    if (idx->n_rows <= 0 || (!ga.scopes && ga.n_ids == 0)) return ORR_OK;
    ORR_TRY(bind_device(idx));
    std::vector<std::vector<int32_t>> members((size_t)G);
    for (int32_t b = 0; b < B; ++b) members[(size_t)ga.query_group[b]].push_back(b);
    // ---- the groups that can be used at all; one of them: the masked call itself, nothing new runs
    int32_t named = 0, only = -1;
    for (int32_t g = 0; g < G; ++g)
        if (!members[(size_t)g].empty() && ga.listed(g)) { named += 1; only = g; }
    if (named == 0) return ORR_OK;
    if (named == 1 && (int32_t)members[(size_t)only].size() == B)        // (whole: the vectors stay where they are)
        return masked_sub_batch(idx, call, ga, only, members[(size_t)only], out_rows, out_scores, out_counts);
    // (sub-batches are gathered on the host, and gathered again by the passes they take: device-resident vectors come down once)
    BatchArgs orig = call;
    std::vector<float> q_down;
    if (call.dim > 0 && is_device_pointer(call.q)) {
        q_down.resize((size_t)B * (size_t)call.dim);
        HIP_TRY(hipMemcpy(q_down.data(), call.q, sizeof(float) * q_down.size(), hipMemcpyDeviceToHost));
        orig.q = q_down.data();
    }
    if (named == 1) return masked_sub_batch(idx, orig, ga, only, members[(size_t)only], out_rows, out_scores, out_counts);
    std::vector<int64_t> took;
    if (ga.scopes)
        for (int32_t g = 0; g < G; ++g) took.push_back(group::took_of(ga.scopes[g]->live.load(), call.candidate_limit));
    GroupFront f;
    ORR_TRY(grouped_front(idx, call, ga, members, took.data(), f));
    if (f.n_used == 0) return ORR_OK;
    if (f.n_used == 1) return masked_sub_batch(idx, orig, ga, f.only, members[(size_t)f.only], out_rows, out_scores, out_counts);
    const group::Plan &plan = f.plan;
    // ---- list groups, and every used group where the grouped pass does not run: a masked call of their own (first: pass_mode
    // tells what ran last)
    for (int32_t g = 0; g < G; ++g) {
        const group::Role role = plan.role[(size_t)g];
        if (role == group::Role::Unused || (plan.grouped && role == group::Role::Screen)) continue;
        ORR_TRY(masked_sub_batch(idx, orig, ga, g, members[(size_t)g], out_rows, out_scores, out_counts));
    }
    // ---- the grouped pass over the screen groups' queries, in slices
    if (!f.screened.empty()) {
        ORR_TRY(grouped_front_upload(idx, call, f));
        const std::vector<int32_t> &screened = f.screened;
        const int32_t per = group::screen_slice((int32_t)screened.size(), plan.max_sample);
        for (size_t b0 = 0; b0 < screened.size(); b0 += (size_t)per)
            ORR_TRY(grouped_screen_ladder(idx, orig, ga, f.gs, f.ms,
                                          std::vector<int32_t>(screened.begin() + b0, screened.begin() + std::min(screened.size(), b0 + (size_t)per)),
                                          out_rows, out_scores, out_counts));
    }
    return ORR_OK;
}

// The best kprime records of each query out of the exact-dot records of P parts ([P][nb][K + 1], as shards' records are laid out:
// one AllRecords pass, or the parts of the list path), ranked by the exact key on the host, with the trailer orr_search_shard
// leaves.  What the reduction drops scores no better than the worst kept record (bound 0); what a part's own selection cut
// keeps that part's cut-off, bound and overflow flag; order_key adds up to the rows that took part.
void reduce_part_records(const orr_candidate *recs, int32_t P, int32_t nb, int64_t K, int32_t kprime, bool use_cos, const double *norms,
                         const std::vector<int32_t> &n_terms, int64_t now_ticks, orr_candidate *out)
{
    std::vector<std::pair<Ranked, const orr_candidate *>> ranked;
    for (int32_t b = 0; b < nb; ++b) {
        orr_candidate *o = out + (size_t)b * ((size_t)kprime + 1);
        orr_candidate t = recs[(size_t)b * ((size_t)K + 1) + (size_t)K];       // part 0's trailer
        // the cut-offs as finish_query reads them: the largest that is a number; NaN (everything left out is NaN too) only alone
        double cut = -std::numeric_limits<double>::infinity();
        bool nan_cut = false;
        auto add_cut = [&](double c) { if (c != c) nan_cut = true; else if (c > cut) cut = c; };
        add_cut(t.approx_score);
        ranked.clear();
        for (int32_t j = 0; j < P; ++j) {
            const orr_candidate *in = recs + ((size_t)j * (size_t)nb + (size_t)b) * ((size_t)K + 1);
            const orr_candidate &tj = in[K];
            for (int32_t i = 0; i < tj.matches; ++i) {
                if (in[i].row_id < 0 && in[i].order_key < 0) continue;
                Ranked r;
                r.score = exact_score(in[i], use_cos, use_cos ? norms[b] : 0.0, n_terms[(size_t)b], now_ticks);
                r.order_key = in[i].order_key;
                r.row_id = in[i].row_id;
                ranked.push_back({r, &in[i]});
            }
            if (j == 0) continue;
            t.order_key += tj.order_key;
            t.flags |= tj.flags & ORR_CAND_OVERFLOW;
            t.dot = std::max(t.dot, tj.dot);
            add_cut(tj.approx_score);
        }
        std::sort(ranked.begin(), ranked.end(), [](const std::pair<Ranked, const orr_candidate *> &x, const std::pair<Ranked, const orr_candidate *> &y) { return ranks_before(x.first, y.first); });
        const int32_t n = (int32_t)ranked.size(), kept = std::min<int32_t>(n, kprime);
        for (int32_t i = 0; i < kprime; ++i) {
            if (i < kept) {
                o[i] = *ranked[(size_t)i].second;
                o[i].approx_score = ranked[(size_t)i].first.score;
            } else {
                memset(&o[i], 0, sizeof(o[i]));
                o[i].row_id = -1; o[i].order_key = -1;
            }
        }
        t.matches = kept;
        if (n > kprime) add_cut(ranked[(size_t)kept - 1].first.score);
        t.approx_score = cut == -std::numeric_limits<double>::infinity() && nan_cut ? std::numeric_limits<double>::quiet_NaN() : cut;
        o[kprime] = t;
    }
}

std::vector<int32_t> term_counts(const uint32_t *query_term_off, int32_t nb)
{
    std::vector<int32_t> n((size_t)nb);
    for (int32_t b = 0; b < nb; ++b) n[(size_t)b] = (int32_t)(query_term_off[b + 1] - query_term_off[b]);
    return n;
}

// orr_search_shard_scoped on the lane the caller holds: one pass at the caller's k', no ladder (the caller's merge certifies).
int scoped_shard(orr_index *idx, const BatchArgs &orig, const ScopeArgs &sc, int32_t kprime, orr_candidate *out)
{
    const int32_t B = orig.B;
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    const size_t rec_q = (size_t)kprime + 1;
    std::vector<int64_t> limit((size_t)B);
    for (int32_t b = 0; b < B; ++b)
        limit[(size_t)b] = std::max<int64_t>(0, std::max<int64_t>(1, orig.candidate_limit) - (sc.before ? std::max<int64_t>(0, sc.before[b]) : 0));
    ORR_TRY(bind_device(idx));
    if (idx->n_rows <= 0 || sc.n_ids == 0) {           // nothing on this shard takes part: empty records + trailers
        HIP_TRY(hipMemcpy(out, empty_records(B, kprime).data(), sizeof(orr_candidate) * (size_t)B * rec_q, hipMemcpyDefault));
        return ORR_OK;
    }
    ORR_TRY(ensure_scope_table(idx));
    const bool all = kprime > orr::kSelWidth;          // (AllRecords: at least k' records per query, so that the reduction has its slots)
    const int32_t per = scope_slice_width(idx, B);
    std::vector<orr_candidate> reduced;
    for (int32_t b0 = 0; b0 < B; b0 += per) {
        ScopeSlice sl;
        ORR_TRY(open_scope_slice(idx, sc, limit, b0, per, "orr_search_shard_scoped", sl));
        std::vector<uint32_t> q((size_t)sl.nq);
        std::iota(q.begin(), q.end(), 0u);
        ORR_TRY(for_each_scoped_part(idx, orig, sl, q, all ? scope::Form::AllRecords : scope::Form::Selection, kprime, [&](const ScopedPart &pt) -> int {
            const size_t nb = pt.ids.size();
            if (all) {
                reduced.resize(nb * rec_q);
                reduce_part_records(pt.recs, 1, (int32_t)nb, pt.kprime, kprime, use_cos, idx->h_norm_a.data(), term_counts(pt.cur.query_term_off, (int32_t)nb),
                                    pt.cur.now_ticks, reduced.data());
            }
            HIP_TRY(hipMemcpy(out + (size_t)pt.ids[0] * rec_q, all ? reduced.data() : pt.recs, sizeof(orr_candidate) * nb * rec_q, hipMemcpyDefault));
            return ORR_OK;
        }));
    }
    return ORR_OK;
}

// orr_index_scope_count on the lane the caller holds: out_live[b] = the live rows query b's scope resolves to on this shard.
int scope_count_on_lane(orr_index *idx, int32_t B, const ScopeArgs &sc, int64_t *out_live)
{
    for (int32_t b = 0; b < B; ++b) out_live[b] = 0;
    if (idx->n_rows <= 0 || sc.n_ids == 0) return ORR_OK;
    ORR_TRY(bind_device(idx));
    ORR_TRY(ensure_scope_table(idx));
    const std::vector<int64_t> limit((size_t)B, std::numeric_limits<int64_t>::max());
    const int32_t per = scope_slice_width(idx, B);
    for (int32_t b0 = 0; b0 < B; b0 += per) {
        ScopeSlice sl;
        ORR_TRY(build_scope_slice(idx, sc, limit, b0, std::min<int32_t>(per, B - b0), sl));
        for (int32_t i = 0; i < sl.nq; ++i) out_live[b0 + i] = (int64_t)sl.live[i];
    }
    return ORR_OK;
}

// ---- orr_search_shard_masked: the record form of the masked search, one pass at the caller's k' ----------------------------

// The list path of the shard form for the queries `ids` of the call (ascending): one rung of the list path in parts
// (list_part_records) at k' -- beyond a selection list the all-records form -- and the parts' records reduced to k' per query.
// One part within a list is what the scoped pass wrote, trailer included.
int masked_shard_list(orr_index *idx, const BatchArgs &orig, const ScopeSlice &sl, const MaskScope &ms, const std::vector<int32_t> &ids,
                      int32_t kprime, orr_candidate *out)
{
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    const bool all = kprime > orr::kSelWidth;
    const int64_t part_rows = idx->opt_mask_part_rows;
    const int64_t P = mask::part_count(ms.took, part_rows);
    if (P > (1 << 16)) return fail(ORR_EINVAL, "orr_search_shard_masked: mask_part_rows %lld cuts the scope into %lld parts", (long long)part_rows, (long long)P);
    const int64_t K = all ? std::max<int64_t>({(int64_t)1, std::min<int64_t>(ms.took, part_rows)}) : (int64_t)kprime;   // records per query and part
    const size_t rec_q = (size_t)kprime + 1;
    const int32_t n_ids = (int32_t)ids.size();
    const int32_t group = mask::merge_group(n_ids, P, K, mask::kMergeBudgetBytes);
    std::vector<orr_candidate> store, reduced;
    std::vector<double> norms;
    for (int32_t g0 = 0; g0 < n_ids; g0 += group) {
        const std::vector<int32_t> gids(ids.begin() + g0, ids.begin() + std::min<int32_t>(n_ids, g0 + group));
        const int32_t nb = (int32_t)gids.size();
        ORR_TRY(list_part_records(idx, orig, sl, ms, gids, all ? scope::Form::AllRecords : scope::Form::Selection, K, false, store, norms));
        const orr_candidate *recs = store.data();
        if (all || P > 1) {
            std::vector<int32_t> n_terms((size_t)nb);
            for (int32_t i = 0; i < nb; ++i) n_terms[(size_t)i] = (int32_t)(orig.query_term_off[gids[(size_t)i] + 1] - orig.query_term_off[gids[(size_t)i]]);
            reduced.resize((size_t)nb * rec_q);
            reduce_part_records(store.data(), (int32_t)P, nb, K, kprime, use_cos, norms.data(), n_terms, orig.now_ticks, reduced.data());
            recs = reduced.data();
        }
        for (int32_t i = 0; i < nb; ++i)
            HIP_TRY(hipMemcpy(out + (size_t)gids[(size_t)i] * rec_q, recs + (size_t)i * rec_q, sizeof(orr_candidate) * rec_q, hipMemcpyDefault));
    }
    return ORR_OK;
}

// The queries `ids` of the call (ascending) through ONE masked screen at k'; the queries whose survivors' buffers overflowed
// repeat once, inside the call, with buffers sized from the measured counts (shard_pass_into's growth).  A pass plan_form finds
// no two-stage form for goes down the list path.
int masked_shard_screen(orr_index *idx, const BatchArgs &orig, const ScopeSlice &sl, const MaskScope &ms, const std::vector<int32_t> &ids,
                        int32_t kprime, orr_candidate *out)
{
    const size_t rec_q = (size_t)kprime + 1;
    std::vector<int32_t> active = ids;
    for (int round = 0; round < 2; ++round) {
        const size_t nb = active.size();
        SubBatch sb;
        BatchArgs cur;
        ORR_TRY(build_subset(idx, orig, active, sb, cur));
        PassPlan pass;
        const float *q_host = nullptr;
        const orr_candidate *recs = nullptr;
        const int rc = retry_pass(idx, [&] { return run_masked_pass(idx, cur, kprime, ms, &q_host, &recs, pass); });
        if (rc == kNotMaskable) return masked_shard_list(idx, orig, sl, ms, active, kprime, out);
        if (rc != ORR_OK) return rc;
        for (size_t i = 0; i < nb; ++i)
            HIP_TRY(hipMemcpy(out + (size_t)active[i] * rec_q, recs + i * rec_q, sizeof(orr_candidate) * rec_q, hipMemcpyDefault));
        const ShardOutcome o = outcome_of(idx, pass, ms.n_clip);
        idx->sstats.passes += 1;
        if (round > 0) idx->sstats.requeried += (int64_t)nb;
        escalation::account_survivors(idx->sstats, o, nb);
        if (round > 0 || !o.kept(nb)) break;
        std::vector<int32_t> over;
        uint32_t worst = 0, cap = 0;
        for (size_t i = 0; i < nb; ++i)
            if (o.overflowed(i)) { over.push_back(active[i]); worst = std::max(worst, o.survivors[i]); }
        if (over.empty() || !escalation::grown_survivor_cap(o.pass_cap, worst, ms.n_clip, over.size(), &cap)) break;     // the caller's escalation
        idx->sstats.buffer_growths += 1;                       // the index keeps the larger size, as for the unscoped search
        if (cap > idx->survivor_cap) idx->survivor_cap = cap;
        if (!idx->is_view || idx->internal_lane) publish_survivor_hint(const_cast<orr_index *>(owner_of(idx)), cap);
        active.swap(over);
    }
    return ORR_OK;
}

// orr_search_shard_masked on the lane the caller holds: one pass at the caller's k', no ladder (the caller's merge certifies).
// orig.topk: the k the floor's sample serves.  The scope is a list, resolved here, or a handle the caller holds shared
// (orr_search_shard_in_scope): then nothing is resolved, as in masked_batch.
int masked_shard(orr_index *idx, const BatchArgs &orig, const ScopeSource &src, int64_t scope_before, int32_t kprime, int32_t pass, orr_candidate *out)
{
    const int32_t B = orig.B;
    const bool use_cos = orig.dim > 0 && orig.dim == idx->dim;
    const size_t rec_q = (size_t)kprime + 1;
    const int64_t limit = cscope::shard_limit(orig.candidate_limit, scope_before);
    ORR_TRY(bind_device(idx));
    auto nothing = [&]() -> int {                      // nothing on this shard takes part: empty records + trailers
        HIP_TRY(hipMemcpy(out, empty_records(B, kprime).data(), sizeof(orr_candidate) * (size_t)B * rec_q, hipMemcpyDefault));
        return ORR_OK;
    };
    if (idx->n_rows <= 0 || src.empty() || limit == 0) return nothing();
    if (src.list) ORR_TRY(ensure_scope_table(idx));
    ScopeSlice sl;
    MaskScope ms;
    ORR_TRY(resolve_mask_scope(idx, B, orig.topk, src, limit, sl, ms));
    if (ms.took == 0) return nothing();
    std::vector<int32_t> ids((size_t)B);
    std::iota(ids.begin(), ids.end(), 0);
    const bool eligible = mask::eligible(use_cos, idx->dim, orig.topk, orr::kSelWidth, ms.n_clip, idx->opt_two_stage, ms.took);
    if (pass != 0 || kprime > orr::kSelWidth || mask::choose(idx->opt_mask_screen, eligible, B, ms.took, ms.n_clip) == mask::Path::List)
        return masked_shard_list(idx, orig, sl, ms, ids, kprime, out);
    const int32_t per = mask::screen_slice(B, ms.sample);
    for (int32_t b0 = 0; b0 < B; b0 += per)
        ORR_TRY(masked_shard_screen(idx, orig, sl, ms, std::vector<int32_t>(ids.begin() + b0, ids.begin() + std::min<int32_t>(B, b0 + per)), kprime, out));
    return ORR_OK;
}

// ---- orr_search_shard_in_scopes: the record form of the grouped search over handles, one pass at the caller's k' ------------

// The queries `ids` of the call (ascending, all of group g) through the masked shard form of their group, the records
// scattered into out.
int grouped_shard_own(orr_index *idx, const BatchArgs &orig, const GroupArgs &ga, int32_t g, const std::vector<int32_t> &ids,
                      int64_t scope_before, int32_t kprime, int32_t pass, orr_candidate *out)
{
    if (ids.empty()) return ORR_OK;
    const size_t rec_q = (size_t)kprime + 1;
    const ScopeSource src{nullptr, ga.scopes[g]};
    SubBatch sb;
    BatchArgs cur;
    ORR_TRY(build_subset(idx, orig, ids, sb, cur));
    if (cur.B == orig.B) return masked_shard(idx, cur, src, scope_before, kprime, pass, out);       // every query of the call
    std::vector<orr_candidate> recs(ids.size() * rec_q);
    ORR_TRY(masked_shard(idx, cur, src, scope_before, kprime, pass, recs.data()));
    for (size_t i = 0; i < ids.size(); ++i)
        HIP_TRY(hipMemcpy(out + (size_t)ids[i] * rec_q, recs.data() + i * rec_q, sizeof(orr_candidate) * rec_q, hipMemcpyDefault));
    return ORR_OK;
}

// `ids` (ascending) split by group, each part through its group's own masked shard form.
int grouped_shard_owns(orr_index *idx, const BatchArgs &orig, const GroupArgs &ga, const std::vector<int32_t> &ids, const int64_t *scope_before,
                       int32_t kprime, int32_t pass, orr_candidate *out)
{
    std::vector<std::vector<int32_t>> by_group((size_t)ga.n_groups);
    for (int32_t b : ids) by_group[(size_t)ga.query_group[b]].push_back(b);
    for (int32_t g = 0; g < ga.n_groups; ++g)
        ORR_TRY(grouped_shard_own(idx, orig, ga, g, by_group[(size_t)g], scope_before[g], kprime, pass, out));
    return ORR_OK;
}

// The queries `ids` of the call (ascending, all of screen groups) through ONE grouped screen at k'; the queries whose survivors'
// buffers overflowed repeat once, inside the call, with buffers of the call's own (group::next_step).  A pass plan_form finds
// no two-stage form for goes through the groups' own shard forms.
int grouped_shard_screen(orr_index *idx, const BatchArgs &orig, const GroupArgs &ga, GroupScopes &gs, const MaskScope &ms,
                         const std::vector<int32_t> &ids, const int64_t *scope_before, int32_t kprime, orr_candidate *out, bool *ran)
{
    const size_t rec_q = (size_t)kprime + 1;
    std::vector<int32_t> active = ids;
    gs.cap = 0;
    for (int round = 0; round < group::kMaxGroupedPasses; ++round) {
        const size_t nb = active.size();
        SubBatch sb;
        BatchArgs cur;
        ORR_TRY(build_subset(idx, orig, active, sb, cur));
        gs.qgroup.resize(nb);
        for (size_t i = 0; i < nb; ++i) gs.qgroup[i] = ga.query_group[active[i]];
        PassPlan pass;
        const float *q_host = nullptr;
        const orr_candidate *recs = nullptr;
        const int rc = retry_pass(idx, [&] { return run_masked_pass(idx, cur, kprime, ms, &q_host, &recs, pass, &gs); });
        if (rc == kNotMaskable) { gs.cap = 0; return grouped_shard_owns(idx, orig, ga, active, scope_before, kprime, 0, out); }
        if (rc != ORR_OK) { gs.cap = 0; return rc; }
        *ran = true;
        for (size_t i = 0; i < nb; ++i)
            HIP_TRY(hipMemcpy(out + (size_t)active[i] * rec_q, recs + i * rec_q, sizeof(orr_candidate) * rec_q, hipMemcpyDefault));
        const ShardOutcome o = outcome_of(idx, pass, ms.n_clip);       // (survivor_cap: the lane's, which the call's own growth leaves alone)
        idx->sstats.passes += 1;
        if (round > 0) idx->sstats.requeried += (int64_t)nb;
        escalation::account_survivors(idx->sstats, o, nb);
        if (round + 1 >= group::kMaxGroupedPasses || !o.kept(nb)) break;
        std::vector<int32_t> over;
        uint32_t worst = 0;
        for (size_t i = 0; i < nb; ++i)
            if (o.overflowed(i)) { over.push_back(active[i]); worst = std::max(worst, o.survivors[i]); }
        if (over.empty()) break;
        const group::Next nx = group::next_step(true, false, o.pass_cap, worst, ms.n_clip, over.size());
        if (nx.step != group::Step::GrowBuffers) break;                // the caller's escalation
        idx->sstats.buffer_growths += 1;       // the call's own: neither the lane nor the handle keeps the size
        gs.cap = nx.new_cap;
        active.swap(over);
    }
    gs.cap = 0;
    return ORR_OK;
}

// orr_search_shard_in_scopes on the lane the caller holds, the scopes held shared by the caller: one pass at the caller's k', no
// ladder (the caller's merge certifies).  orig.topk: the k the floors' samples serve.  *ran_grouped: a grouped screen ran.
int grouped_shard(orr_index *idx, const BatchArgs &call, const GroupArgs &ga, const int64_t *scope_before, int32_t kprime, int32_t pass,
                  orr_candidate *out, bool *ran_grouped)
{
    const int32_t B = call.B, G = ga.n_groups;
    const size_t rec_q = (size_t)kprime + 1;
    bool ran_here = false;
    bool *ran = ran_grouped ? ran_grouped : &ran_here;
    *ran = false;
    ORR_TRY(bind_device(idx));
    std::vector<std::vector<int32_t>> members((size_t)G);
    for (int32_t b = 0; b < B; ++b) members[(size_t)ga.query_group[b]].push_back(b);
    std::vector<int64_t> took((size_t)G, 0);
    int32_t n_used = 0, only = -1;
    for (int32_t g = 0; g < G; ++g) {
        took[(size_t)g] = idx->n_rows <= 0 ? 0 : cscope::shard_took(ga.scopes[g]->live.load(), call.candidate_limit, scope_before[g]);
        if (!members[(size_t)g].empty() && took[(size_t)g] > 0) { n_used += 1; only = g; }
    }
    // one used group that every query names: the in-scope shard form itself, nothing new runs
    if (n_used == 1 && (int32_t)members[(size_t)only].size() == B) return masked_shard(idx, call, ScopeSource{nullptr, ga.scopes[only]}, scope_before[only], kprime, pass, out);
    // a query whose scope takes no row here: an empty record and trailer (the others are written over below)
    HIP_TRY(hipMemcpy(out, empty_records(B, kprime).data(), sizeof(orr_candidate) * (size_t)B * rec_q, hipMemcpyDefault));
    if (n_used == 0) return ORR_OK;
    // (sub-batches are gathered on the host, and gathered again by the passes they take: device-resident vectors come down once)
    BatchArgs orig = call;
    std::vector<float> q_down;
    if (call.dim > 0 && is_device_pointer(call.q)) {
        q_down.resize((size_t)B * (size_t)call.dim);
        HIP_TRY(hipMemcpy(q_down.data(), call.q, sizeof(float) * q_down.size(), hipMemcpyDeviceToHost));
        orig.q = q_down.data();
    }
    auto own = [&](int32_t g) { return grouped_shard_own(idx, orig, ga, g, members[(size_t)g], scope_before[g], kprime, pass, out); };
    if (n_used == 1) return own(only);
    if (pass != 0 || kprime > orr::kSelWidth) {         // the list path: per group
        for (int32_t g = 0; g < G; ++g)
            if (!members[(size_t)g].empty() && took[(size_t)g] > 0) ORR_TRY(own(g));
        return ORR_OK;
    }
    GroupFront f;
    ORR_TRY(grouped_front(idx, orig, ga, members, took.data(), f));
    const group::Plan &plan = f.plan;
    for (int32_t g = 0; g < G; ++g) {
        const group::Role role = plan.role[(size_t)g];
        if (role == group::Role::Unused || (plan.grouped && role == group::Role::Screen)) continue;
        ORR_TRY(own(g));
    }
    if (!f.screened.empty()) {
        ORR_TRY(grouped_front_upload(idx, orig, f));
        const std::vector<int32_t> &screened = f.screened;
        const int32_t per = group::screen_slice((int32_t)screened.size(), plan.max_sample);
        for (size_t b0 = 0; b0 < screened.size(); b0 += (size_t)per)
            ORR_TRY(grouped_shard_screen(idx, orig, ga, f.gs, f.ms,
                                         std::vector<int32_t>(screened.begin() + b0, screened.begin() + std::min(screened.size(), b0 + (size_t)per)),
                                         scope_before, kprime, out, ran));
    }
    return ORR_OK;
}

}  // namespace

extern "C" {

int orr_index_search_stats(orr_index *idx, orr_search_stats *out, int32_t reset)
{
    if (!idx) return fail(ORR_EINVAL, "orr_index_search_stats: null index");
    LanePool::Exclusive all(pool_of(idx));
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->sstats.survivor_capacity = idx->survivor_cap;
    idx->sstats.vocab_tokens = idx->n_tokens;
    if (out) {
        *out = idx->sstats;
        for_each_lane(idx, [&](orr_index *l) {         // the counters of every lane of this handle
            if (l == idx) return;
            l->sstats.survivor_capacity = l->survivor_cap;
            escalation::add_search_stats(*out, l->sstats);
        });
    }
    if (reset) {
        auto clear = [](orr_index *x) { const int64_t cap = x->survivor_cap; x->sstats = orr_search_stats{}; x->sstats.survivor_capacity = cap; };
        for_each_lane(idx, clear);
    }
    return ORR_OK;
}

// One shard pass of `a` (all of its queries) with the records written to out[first .. first + a.B) (host or device memory), then --
// inside the call -- the queries whose survivors' buffers overflowed again with buffers sized from the measured counts
// (clustered rows, cosine-only scores): a caller that only saw ORR_CAND_OVERFLOW could but repeat the whole batch through
// the exact pass on every shard.  Caller holds idx->mu.
static int shard_pass_into(orr_index *idx, BatchArgs a, int32_t kprime, int64_t candidate_limit, orr_candidate *out, size_t first,
                           bool dev_out)
{
    const int32_t B = a.B;
    const size_t rec_q = sizeof(orr_candidate) * ((size_t)kprime + 1);
    unsigned char *dst = reinterpret_cast<unsigned char *>(out) + rec_q * first;
    a.out_dev = dev_out ? reinterpret_cast<orr_candidate *>(dst) : nullptr;   // records written where the caller wants them (the all-gather's send buffer)
    PassPlan pass;
    ORR_TRY(run_shard(idx, a, kprime, false, nullptr, nullptr, pass));
    if (!dev_out) HIP_TRY(hipMemcpy(dst, idx->ws_cand.p, rec_q * (size_t)B, hipMemcpyDefault));
    idx->sstats.passes += 1;
    const int64_t n = participating_rows(idx, candidate_limit);
    std::vector<int32_t> active((size_t)B);             // the queries the last pass answered, in the batch's numbering
    std::iota(active.begin(), active.end(), 0);
    for (int round = 0; round < 4; ++round) {
        const ShardOutcome kept = outcome_of(idx, pass, n);
        if (!kept.kept(active.size())) break;
        escalation::account_survivors(idx->sstats, kept, active.size());       // (statistics: only the queries this pass ran)
        std::vector<int32_t> over;
        uint32_t worst = 0, cap = 0;
        for (size_t i = 0; i < active.size(); ++i)
            if (kept.overflowed(i)) { over.push_back(active[i]); worst = std::max(worst, kept.survivors[i]); }
        if (over.empty() || !escalation::grown_survivor_cap(kept.pass_cap, worst, n, over.size(), &cap)) break;   // the caller's escalation
        if (cap > idx->survivor_cap) idx->survivor_cap = cap;
        idx->sstats.buffer_growths += 1;
        SubBatch sb;
        BatchArgs sub;
        a.out_dev = nullptr;
        ORR_TRY(build_subset(idx, a, over, sb, sub));
        ORR_TRY(run_shard(idx, sub, kprime, false, nullptr, nullptr, pass));    // records in idx->ws_cand
        idx->sstats.passes += 1; idx->sstats.requeried += (int64_t)over.size();
        for (size_t i = 0; i < over.size(); ++i)
            HIP_TRY(hipMemcpy(dst + rec_q * (size_t)over[i], static_cast<const unsigned char *>(idx->ws_cand.p) + rec_q * i, rec_q, hipMemcpyDefault));
        active.swap(over);
    }
    return ORR_OK;
}

// orr_search_shard_ex, or with `sticky` orr_search_shard: topk and pass are then the lane's options "shard_topk" and "shard_pass"
// (every lane carries the options of its index, and they change under Exclusive only: the lane's holder reads them as they are)
static int search_shard(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                        const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                        int64_t candidate_limit, int32_t topk, int32_t pass, bool sticky, orr_candidate *out)
{
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, kprime};
    ORR_TRY(check_batch(idx, a, "orr_search_shard"));
    if (kprime < 1) return fail(ORR_EINVAL, "orr_search_shard: kprime must be >= 1");
    if (!out) return fail(ORR_EINVAL, "orr_search_shard: out is NULL");
    if (pass < 0 || pass > 2 || topk < 0) return fail(ORR_EINVAL, "orr_search_shard_ex: pass takes 0, 1 or 2 and topk must be >= 0");
    Lane ln = acquire_lane(idx);                       // concurrent calls on one handle run on different lanes
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    if (sticky) { topk = idx->opt_shard_topk; pass = idx->opt_shard_pass; }
    // the caller's escalation after a merge that could not certify every query (orr_merge_candidates)
    a.no_fuse = pass >= 1;
    a.force_exact = pass >= 2;
    // the floor of the two-stage pass: from the k-th best of the sample when the caller told its topK (valid across shards:
    // the global k-th best is at least every shard's), else from the k'-th
    if (topk > 0) a.topk = std::min<int32_t>(kprime, topk);
    const bool dev_out = is_device_pointer(out);
    idx->sstats.searches += 1; idx->sstats.queries += B;
    // passes that keep one number per (query,row) -- the unfused and the exact one -- run over slices of the batch, so that
    // their workspace stays bounded whatever the batch (1024 queries x 12.5M rows x 8 B = 102 GB in one piece)
    const int32_t per = escalation::slice_width(B, participating_rows(idx, candidate_limit), pass >= 1);
    if (per == 0) return shard_pass_into(idx, a, kprime, candidate_limit, out, 0, dev_out);
    for (int32_t b0 = 0; b0 < B; b0 += per) {
        std::vector<int32_t> part((size_t)std::min<int32_t>(per, B - b0));
        std::iota(part.begin(), part.end(), b0);
        SubBatch sb;
        BatchArgs sub;
        ORR_TRY(build_subset(idx, a, part, sb, sub));
        ORR_TRY(shard_pass_into(idx, sub, kprime, candidate_limit, out, (size_t)b0, dev_out));
    }
    return ORR_OK;
}

int orr_search_shard(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                     const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                     int64_t candidate_limit, orr_candidate *out)
{
    // the sticky per-index forms of the two arguments ("shard_topk", "shard_pass"); orr_search_shard_ex takes them per call
    return search_shard(idx, B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, kprime, candidate_limit, 0, 0, true, out);
}

int orr_search_shard_ex(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                        const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                        int64_t candidate_limit, int32_t topk, int32_t pass, orr_candidate *out)
{
    return search_shard(idx, B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, kprime, candidate_limit, topk, pass, false, out);
}

int orr_merge_candidates(int32_t n_shards, int32_t B, int32_t kprime, const orr_candidate *all, int32_t index_dim,
                         int32_t dim, const float *q_host, const uint32_t *query_term_off, int64_t now_ticks,
                         int32_t topk, int64_t *out_rows, double *out_scores, int32_t *out_counts,
                         int32_t *out_uncertified)
{
    return orr_merge_candidates_ex(n_shards, B, kprime, all, index_dim, dim, q_host, query_term_off, now_ticks, topk, out_rows,
                                   out_scores, out_counts, out_uncertified, nullptr);
}

int orr_merge_candidates_ex(int32_t n_shards, int32_t B, int32_t kprime, const orr_candidate *all, int32_t index_dim,
                            int32_t dim, const float *q_host, const uint32_t *query_term_off, int64_t now_ticks,
                            int32_t topk, int64_t *out_rows, double *out_scores, int32_t *out_counts,
                            int32_t *out_uncertified, uint8_t *out_certified)
{
    if (n_shards < 1 || B < 1 || kprime < 1) return fail(ORR_EINVAL, "orr_merge_candidates: sizes must be positive");
    if (!all || !query_term_off || !out_rows || !out_scores) return fail(ORR_EINVAL, "orr_merge_candidates: null argument");
    if (dim < 0 || index_dim < 0) return fail(ORR_EINVAL, "orr_merge_candidates: negative dimension");
    const bool use_cos = dim > 0 && dim == index_dim;
    if (use_cos && !q_host) return fail(ORR_EINVAL, "orr_merge_candidates: q_host is required with dim %d", dim);
    return merge_impl(n_shards, B, kprime, all, dim, use_cos, q_host, nullptr, query_term_off, now_ticks, topk, out_rows,
                      out_scores, out_counts, out_uncertified, out_certified);
}

int orr_search_batch(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                     const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                     int64_t candidate_limit, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    ORR_TRY(check_batch(idx, a, "orr_search_batch"));
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "orr_search_batch: output buffers are required");
    Lane ln = acquire_lane(idx);                       // concurrent calls on one handle run on different lanes
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    const int32_t take = std::max<int32_t>(1, topk);
    const int64_t n = participating_rows(idx, candidate_limit);

    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    const int r = escalate(index_backend(idx, "orr_search_batch", n), a, escalation::initial_kprime(take, n, orr::kSelWidth),
                           out_rows, out_scores, out_counts);
    g_ht.done();
    return r;
}

int orr_search_batch_scoped(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                            const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                            int64_t candidate_limit, int64_t n_scope_ids, const int64_t *scope_ids, const uint64_t *scope_off,
                            int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    const ScopeArgs sc{n_scope_ids, scope_ids, scope_off, nullptr};
    ORR_TRY(check_scope(idx, B, sc, "orr_search_batch_scoped"));
    ORR_TRY(check_batch(idx, a, "orr_search_batch_scoped"));
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "orr_search_batch_scoped: output buffers are required");
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return scoped_batch(idx, a, sc, out_rows, out_scores, out_counts);
}

int orr_search_batch_masked(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                            const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                            int64_t candidate_limit, int64_t n_scope_ids, const int64_t *scope_ids,
                            int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    const ScopeArgs sc{n_scope_ids, scope_ids, nullptr, nullptr};
    ORR_TRY(check_scope(idx, B, sc, "orr_search_batch_masked"));
    ORR_TRY(check_batch(idx, a, "orr_search_batch_masked"));
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "orr_search_batch_masked: output buffers are required");
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return masked_batch(idx, a, ScopeSource{&sc, nullptr}, out_rows, out_scores, out_counts);
}

int orr_search_batch_masked_groups(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                                   const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                   int64_t candidate_limit, int32_t n_groups, int64_t n_scope_ids, const int64_t *scope_ids,
                                   const uint64_t *group_off, const int32_t *query_group,
                                   int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    static const char *fn = "orr_search_batch_masked_groups";
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    const ScopeArgs sc{n_scope_ids, scope_ids, nullptr, nullptr};
    ORR_TRY(check_scope(idx, B, sc, fn));
    ORR_TRY(check_batch(idx, a, fn));
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "%s: output buffers are required", fn);
    if (!group::groups_valid(n_groups)) return fail(ORR_EINVAL, "%s: n_groups must be in 1 .. %d", fn, group::kMaxGroups);
    if (!group_off) return fail(ORR_EINVAL, "%s: group_off is NULL", fn);
    if (!query_group) return fail(ORR_EINVAL, "%s: query_group is NULL", fn);
    if (!scope::offsets_valid(group_off, n_groups, n_scope_ids))
        return fail(ORR_EINVAL, "%s: group_off must start at 0, never decrease and end at n_scope_ids", fn);
    if (!group::assignment_valid(query_group, B, n_groups))
        return fail(ORR_EINVAL, "%s: query_group must name a group in 0 .. %d for every query", fn, n_groups - 1);
    const GroupArgs ga{n_groups, n_scope_ids, scope_ids, group_off, query_group};
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return grouped_batch(idx, a, ga, out_rows, out_scores, out_counts);
}

// ---- scope handles (orr_scope): the resolve of a masked search, kept ---------------------------------------------------------

// The shard of a scope, or the reason it cannot be used: ORR_ESTATE orphaned; with idx: ORR_EINVAL another shard.
static int scope_owner(const orr_scope *sc, const orr_index *idx, const char *fn, orr_index **own)
{
    *own = sc->owner.load();
    if (!*own) return fail(ORR_ESTATE, "%s: the scope is orphaned: its index was destroyed", fn);
    if (idx && owner_of(idx) != *own) return fail(ORR_EINVAL, "%s: the scope belongs to another shard", fn);
    return ORR_OK;
}

// ids (host or device) -> their live rows' bits OR-ed into the scope's bitmap, on the lane the caller holds
static int scope_or_ids(orr_index *lane, orr_scope *sc, int64_t n_ids, const int64_t *ids)
{
    if (n_ids <= 0 || lane->n_rows <= 0) return ORR_OK;
    ORR_TRY(ensure_scope_table(lane));
    const orr_index *own = owner_of(lane);
    ORR_TRY(lane->ws_scope_ids.reserve(sizeof(int64_t) * (size_t)n_ids));
    HIP_TRY(hipMemcpyAsync(lane->ws_scope_ids.p, ids, sizeof(int64_t) * (size_t)n_ids, hipMemcpyDefault, lane->stream));
    Timed t(lane, "scope_handle_lookup", 8.0 * (double)n_ids);
    HIP_TRY(orr::launch_scope_lookup(own->scope_tab_ids, own->scope_tab_pos, lane->n_rows, lane->ws_scope_ids.as<int64_t>(), n_ids, nullptr, 1,
                                     own->d_dead.as<int64_t>(), (int32_t)own->dead.size(), sc->bm, sc->words, lane->stream));
    return ORR_OK;
}

// A new scope over the lane's shard filled by fill(scope), counted, and registered with the owning index.
static int make_scope(orr_index *idx, const char *fn, orr_scope **out, const std::function<int(orr_index *, orr_scope *)> &fill)
{
    Lane ln = acquire_lane(idx);                       // the lookup runs like a search: its own lane, beside the others
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    if (!lane->sealed) return fail(ORR_ESTATE, "%s: the index is not sealed", fn);
    ORR_TRY(bind_device(lane));
    orr_scope *sc = new (std::nothrow) orr_scope();
    if (!sc) return fail(ORR_ENOMEM, "out of host memory");
    sc->n_rows = lane->n_rows;
    int r = alloc_scope_arrays(sc->n_rows, &sc->bm, &sc->chunks, &sc->words);
    if (r == ORR_OK) r = fill(lane, sc);
    if (r == ORR_OK) r = refresh_scope(lane, sc);
    if (r != ORR_OK) {
        (void)hipStreamSynchronize(lane->stream);
        free_scope_arrays(sc->bm, sc->chunks);
        delete sc;
        return r;
    }
    orr_index *own = const_cast<orr_index *>(owner_of(lane));
    sc->owner.store(own);
    { std::lock_guard<std::mutex> g(own->scope_mu); own->scopes.push_back(sc); }
    *out = sc;
    return ORR_OK;
}

int orr_scope_create(orr_index *idx, int64_t n_ids, const int64_t *ids, orr_scope **out)
{
    if (!out) return fail(ORR_EINVAL, "orr_scope_create: out is NULL");
    if (n_ids < 0) return fail(ORR_EINVAL, "orr_scope_create: n_ids is negative");
    if (n_ids > 0 && !ids) return fail(ORR_EINVAL, "orr_scope_create: ids is NULL with %lld ids", (long long)n_ids);
    if (!idx) return fail(ORR_EINVAL, "orr_scope_create: null index");
    return make_scope(idx, "orr_scope_create", out, [&](orr_index *lane, orr_scope *sc) -> int {
        HIP_TRY(hipMemsetAsync(sc->bm, 0, sizeof(uint32_t) * (size_t)sc->words, lane->stream));
        return scope_or_ids(lane, sc, n_ids, ids);
    });
}

int orr_scope_create_ticks(orr_index *idx, int64_t ticks_from, int64_t ticks_to, orr_scope **out)
{
    if (!out) return fail(ORR_EINVAL, "orr_scope_create_ticks: out is NULL");
    if (!idx) return fail(ORR_EINVAL, "orr_scope_create_ticks: null index");
    return make_scope(idx, "orr_scope_create_ticks", out, [&](orr_index *lane, orr_scope *sc) -> int {
        const orr_index *own = owner_of(lane);         // the host mirror of the timestamps and the deleted set live there
        const auto range = scope_set::ticks_range(own->h_created.data(), std::min<int64_t>((int64_t)own->h_created.size(), lane->n_rows), ticks_from, ticks_to);
        {
            Timed t(lane, "scope_fill_range", 4.0 * (double)sc->words);
            HIP_TRY(orr::launch_scope_fill_range(sc->bm, sc->words, range.first, range.second, lane->stream));
        }
        Timed t(lane, "scope_clear_positions", 12.0 * (double)own->dead.size());
        HIP_TRY(orr::launch_scope_clear_positions(sc->bm, sc->words, own->d_dead.as<int64_t>(), (int64_t)own->dead.size(), lane->stream));
        return ORR_OK;
    });
}

// The fill of a term scope (orr_scope_terms_plan.h), on the lane the caller holds:
//   1. the keyword chain of a search for ONE query that owns every term (launch_keyword_side, as it is): a row bitmap per
//      DISTINCT term, its own or -- where the term's only hit is a token with a stored bitmap -- an alias into the token store;
//   2. scope_terms_combine behind it on the keyword stream: the bitmaps folded into the scope's, every word written;
//   3. the hit list checked as finish_pass checks it (check_hit_list): too short, and the bitmaps are incomplete -- the list
//      grows and the chain runs again, a scope is never made of a truncated list;
//   4. the lane left as a search leaves it (clean_keyword_side), whether the chain stands or runs again;
//   5. the deleted rows cleared on the scope's own stream, behind an event: posting lists keep deleted positions until compaction.
// The search statistics do not move (this is no search); the kernel statistics record the launches.
static int scope_fill_terms_run(orr_index *lane, orr_scope *sc, int32_t n_terms, const uint8_t *terms_utf8, const uint32_t *term_off, int32_t mode)
{
    if (n_terms == 0 || lane->n_rows <= 0) {           // nothing to fold: the empty scope
        HIP_TRY(hipMemsetAsync(sc->bm, 0, sizeof(uint32_t) * (size_t)sc->words, lane->stream));
        return ORR_OK;
    }
    const orr_index *own = owner_of(lane);
    const uint32_t query_term_off[2] = {0u, (uint32_t)n_terms};
    BatchArgs a{1, 0, nullptr, terms_utf8, term_off, query_term_off, 0, 0};
    const std::vector<uint32_t> qoff(query_term_off, query_term_off + 2);
    hipStream_t k = lane->stream_kw;
    for (int attempt = 0;; ++attempt) {
        KwSide kws;
        ORR_TRY(launch_keyword_side(lane, a, qoff, kws));
        const int64_t words = kws.view.words_per_term;
        if (words != sc->words || kws.bm_bytes == 0 || kws.bm_bytes % (sizeof(uint32_t) * (size_t)words) != 0)
            return fail(ORR_ESTATE, "orr_scope_create_terms: the keyword side's bitmaps have %lld words, the scope's %lld", (long long)words, (long long)sc->words);
        const int32_t n_distinct = (int32_t)(kws.bm_bytes / (sizeof(uint32_t) * (size_t)words));
        // 16-byte vectors: words % 4 == 0 and each base is t * words, or the token store (tok_bm_words == words) seen from the bitmaps
        if (words % 4 != 0 || (reinterpret_cast<uintptr_t>(kws.view.bitmaps) & 15u) || (reinterpret_cast<uintptr_t>(lane->tok_bm.p) & 15u))
            return fail(ORR_ESTATE, "orr_scope_create_terms: a term bitmap is not 16-byte aligned");
        ORR_TRY(lane->ws_scope_terms.reserve(sizeof(int64_t) * (size_t)scope_terms::kMaxTerms));
        int64_t *h_base = nullptr;                     // the host's copy of the bases: only the statistics read it
        if (lane->profiling == 1) {
            ORR_TRY(lane->pin_scope_terms.reserve(sizeof(int64_t) * (size_t)scope_terms::kMaxTerms));
            h_base = lane->pin_scope_terms.as<int64_t>();
        }
        {
            Timed t(lane, "scope_terms_bases", 24.0 * (double)n_distinct, k);
            HIP_TRY(orr::launch_scope_terms_bases(kws.view.term_word_off, n_distinct, words, lane->ws_scope_terms.as<int64_t>(), h_base, k));
        }
        {
            Timed t(lane, "scope_terms_combine", 4.0 * (double)words * ((double)n_distinct + 1.0), k);
            HIP_TRY(orr::launch_scope_terms_combine(kws.view.bitmaps, lane->ws_scope_terms.as<int64_t>(), n_distinct, mode, words, lane->n_rows, sc->bm, k));
        }
        HIP_TRY(hipEventRecord(lane->ev_kw_done, k));
        HIP_TRY(hipStreamSynchronize(k));              // the bitmaps are read: they may be cleared; the hit count is in pinned memory
        const int verdict = check_hit_list(lane, kws, "orr_scope_create_terms");
        if (verdict != ORR_OK && verdict != kRetryPass) return verdict;
        ORR_TRY(clean_keyword_side(lane, kws, (uint32_t)n_terms));
        if (verdict == kRetryPass) {
            if (attempt + 1 >= keyword::kMaxRuns) return hit_list_kept_overflowing("orr_scope_create_terms");
            continue;
        }
        if (h_base) {                  // what the fold read from STORED token bitmaps (aliased terms: nothing was expanded for them)
            int64_t aliased = 0;
            for (int32_t t = 0; t < n_distinct; ++t) aliased += h_base[t] != (int64_t)t * words;
            lane->stats[(size_t)stat_slot(lane, "scope_terms_aliased")].algo_bytes += 4.0 * (double)words * (double)aliased;
        }
        break;
    }
    HIP_TRY(hipStreamWaitEvent(lane->stream, lane->ev_kw_done, 0));
    Timed t(lane, "scope_clear_positions", 12.0 * (double)own->dead.size());
    HIP_TRY(orr::launch_scope_clear_positions(sc->bm, sc->words, own->d_dead.as<int64_t>(), (int64_t)own->dead.size(), lane->stream));
    return ORR_OK;
}

// ... and whatever it launched on the keyword stream is done before a failed fill's caller frees the scope's bitmap
static int scope_fill_terms(orr_index *lane, orr_scope *sc, int32_t n_terms, const uint8_t *terms_utf8, const uint32_t *term_off, int32_t mode)
{
    const int r = scope_fill_terms_run(lane, sc, n_terms, terms_utf8, term_off, mode);
    if (r != ORR_OK) (void)hipStreamSynchronize(lane->stream_kw);
    return r;
}

int orr_scope_create_terms(orr_index *idx, int32_t n_terms, const uint8_t *terms_utf8, const uint32_t *term_off, int32_t mode, orr_scope **out)
{
    if (!out) return fail(ORR_EINVAL, "orr_scope_create_terms: out is NULL");
    if (!scope_terms::terms_valid(n_terms)) return fail(ORR_EINVAL, "orr_scope_create_terms: n_terms must be in 0 .. %d", scope_terms::kMaxTerms);
    if (n_terms > 0 && (!terms_utf8 || !term_off)) return fail(ORR_EINVAL, "orr_scope_create_terms: terms_utf8 or term_off is NULL with %d terms", n_terms);
    if (!scope_terms::mode_valid(mode)) return fail(ORR_EINVAL, "orr_scope_create_terms: mode must be ORR_TERMS_ALL (0) or ORR_TERMS_ANY (1)");
    const int32_t bad = scope_terms::first_bad_term(term_off, n_terms);
    if (bad >= 0 && term_off[bad + 1] == term_off[bad]) return fail(ORR_EINVAL, "orr_scope_create_terms: term %d is empty", bad);
    if (bad >= 0) return fail(ORR_EINVAL, "orr_scope_create_terms: term_off is not monotone at term %d", bad);
    if (!idx) return fail(ORR_EINVAL, "orr_scope_create_terms: null index");
    return make_scope(idx, "orr_scope_create_terms", out, [&](orr_index *lane, orr_scope *sc) -> int {
        return scope_fill_terms(lane, sc, n_terms, terms_utf8, term_off, mode);
    });
}

// Diagnostic (tests/test_gpu_keyword_chain.py): the keyword chain of a search for ONE query that owns every term, as
// scope_fill_terms_run runs it -- launch_keyword_side as it is, the repeat with a grown hit list, clean_keyword_side -- with the
// per-term bitmaps, the alias flags and the hit count copied out instead of folded.
constexpr int32_t kKwDiagMaxTerms = 4096;
constexpr uint64_t kKwDiagMaxBytes = (uint64_t)1 << 30;

static int keyword_bitmaps_run(orr_index *lane, int32_t n_terms, const uint8_t *terms_utf8, const uint32_t *term_off, int64_t words,
                               uint32_t *out_bitmaps, uint8_t *out_alias, int64_t *out_info)
{
    const uint32_t query_term_off[2] = {0u, (uint32_t)n_terms};
    BatchArgs a{1, 0, nullptr, terms_utf8, term_off, query_term_off, 0, 0};
    const std::vector<uint32_t> qoff(query_term_off, query_term_off + 2);
    hipStream_t k = lane->stream_kw;
    std::vector<int64_t> h_off((size_t)n_terms);
    std::vector<uint8_t> h_alias((size_t)n_terms, 0);
    for (int attempt = 0;; ++attempt) {
        KwSide kws;
        ORR_TRY(launch_keyword_side(lane, a, qoff, kws));
        if (kws.view.words_per_term != words || kws.bm_bytes != sizeof(uint32_t) * (size_t)n_terms * (size_t)words)
            return fail(ORR_ESTATE, "orr_index_keyword_bitmaps: the keyword side made %zu bytes of bitmaps of %lld words for %d terms",
                        kws.bm_bytes, (long long)kws.view.words_per_term, n_terms);
        const bool has_store = kws.view.term_word_off != nullptr && kws.alias != nullptr;
        if (has_store) {
            HIP_TRY(hipMemcpyAsync(h_off.data(), kws.view.term_word_off, sizeof(int64_t) * (size_t)n_terms, hipMemcpyDeviceToHost, k));
            HIP_TRY(hipMemcpyAsync(h_alias.data(), kws.alias, (size_t)n_terms, hipMemcpyDeviceToHost, k));
        }
        HIP_TRY(hipStreamSynchronize(k));              // the chain is done; the hit count is in pinned memory
        const uint32_t hits = (uint32_t)(*lane->pin_kwcnt.as<unsigned long long>() >> 32);
        const int verdict = check_hit_list(lane, kws, "orr_index_keyword_bitmaps");
        if (verdict != ORR_OK && verdict != kRetryPass) return verdict;
        if (verdict == ORR_OK) {      // raw bits, an aliased term's from the token store (term_word_off counts words from the batch's bitmaps)
            HIP_TRY(hipMemcpyAsync(out_bitmaps, kws.view.bitmaps, kws.bm_bytes, hipMemcpyDeviceToHost, k));
            for (int32_t t = 0; has_store && t < n_terms; ++t)
                if (h_off[(size_t)t] != (int64_t)t * words)
                    HIP_TRY(hipMemcpyAsync(out_bitmaps + (size_t)t * (size_t)words, kws.view.bitmaps + h_off[(size_t)t], sizeof(uint32_t) * (size_t)words,
                                           hipMemcpyDeviceToHost, k));
            HIP_TRY(hipStreamSynchronize(k));
        }
        ORR_TRY(clean_keyword_side(lane, kws, (uint32_t)n_terms));
        if (verdict == kRetryPass) {
            if (attempt + 1 >= keyword::kMaxRuns) return hit_list_kept_overflowing("orr_index_keyword_bitmaps");
            continue;
        }
        if (out_alias) memcpy(out_alias, h_alias.data(), (size_t)n_terms);
        out_info[1] = (int64_t)hits;
        out_info[2] = attempt + 1;
        out_info[3] = lane->kw_form_ran;
        break;
    }
    return ORR_OK;
}

int orr_index_keyword_bitmaps(orr_index *idx, int32_t n_terms, const uint8_t *terms_utf8, const uint32_t *term_off, int32_t form, int32_t mid,
                              int64_t out_words_per_term, uint32_t *out_bitmaps, uint8_t *out_alias, int64_t *out_info)
{
    static const char *fn = "orr_index_keyword_bitmaps";
    if (!out_bitmaps || !out_info) return fail(ORR_EINVAL, "%s: out_bitmaps or out_info is NULL", fn);
    if (n_terms < 1 || n_terms > kKwDiagMaxTerms) return fail(ORR_EINVAL, "%s: n_terms must be in 1 .. %d", fn, kKwDiagMaxTerms);
    if (!terms_utf8 || !term_off) return fail(ORR_EINVAL, "%s: terms_utf8 or term_off is NULL", fn);
    if (form < -1 || form > 1) return fail(ORR_EINVAL, "%s: form must be -1 (as a search chooses), 0 (all-pairs) or 1 (lookup)", fn);
    if (mid < -1 || mid > 0) return fail(ORR_EINVAL, "%s: mid must be -1 (default) or 0 (tokens of 17..32 bytes through the wave scan)", fn);
    const int32_t bad = scope_terms::first_bad_term(term_off, n_terms);
    if (bad >= 0 && term_off[bad + 1] == term_off[bad]) return fail(ORR_EINVAL, "%s: term %d is empty", fn, bad);
    if (bad >= 0) return fail(ORR_EINVAL, "%s: term_off is not monotone at term %d", fn, bad);
    {
        std::vector<std::string_view> sorted((size_t)n_terms);
        for (int32_t t = 0; t < n_terms; ++t)
            sorted[(size_t)t] = std::string_view(reinterpret_cast<const char *>(terms_utf8) + term_off[t], term_off[t + 1] - term_off[t]);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(ORR_EINVAL, "%s: the terms are not distinct", fn);
    }
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    Lane ln = acquire_lane(idx);                       // the chain runs like a search's: its own lane, beside the others
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    if (!lane->sealed) return fail(ORR_ESTATE, "%s: the index is not sealed", fn);
    const int64_t words = keyword::words_per_term(lane->n_rows);
    if (out_words_per_term != words) return fail(ORR_EINVAL, "%s: a term bitmap of this shard has %lld words, not %lld", fn, (long long)words, (long long)out_words_per_term);
    if ((uint64_t)n_terms * (uint64_t)words * sizeof(uint32_t) > kKwDiagMaxBytes)
        return fail(ORR_EINVAL, "%s: %d bitmaps of %lld words are more than the %llu bytes a call returns", fn, n_terms, (long long)words, (unsigned long long)kKwDiagMaxBytes);
    out_info[0] = words; out_info[1] = 0; out_info[2] = 0; out_info[3] = -1;
    if (out_alias) memset(out_alias, 0, (size_t)n_terms);
    if (lane->n_rows <= 0) return ORR_OK;
    ORR_TRY(bind_device(lane));
    struct Overrides {                                 // per-call state of the lane: launch_keyword_side reads it ahead of the environment
        orr_index *l;
        ~Overrides() { l->kw_force_form = l->kw_force_mid = -1; }
    } overrides{lane};
    lane->kw_force_form = form;
    lane->kw_force_mid = mid;
    const int r = keyword_bitmaps_run(lane, n_terms, terms_utf8, term_off, words, out_bitmaps, out_alias, out_info);
    if (r != ORR_OK) (void)hipStreamSynchronize(lane->stream_kw);
    collect_events(lane);
    return r;
}

// orr_scope_add_ids behind its locks: the caller holds the lane, its lock and the scope exclusively
static int scope_add_ids_held(orr_index *lane, orr_scope *s, int64_t n_ids, const int64_t *ids, int64_t *out_added)
{
    ORR_TRY(bind_device(lane));
    const int64_t before = s->live.load();
    int r = scope_or_ids(lane, s, n_ids, ids);
    if (r == ORR_OK) r = refresh_scope(lane, s);
    if (r != ORR_OK) { (void)hipStreamSynchronize(lane->stream); return r; }
    if (out_added) *out_added = s->live.load() - before;
    return ORR_OK;
}

// orr_scope_combine behind its locks: the caller holds the lane, its lock, dst exclusively and src shared
static int scope_combine_held(orr_index *lane, orr_scope *dst, int32_t op, const orr_scope *src)
{
    if (dst->words != src->words) return fail(ORR_ESTATE, "orr_scope_combine: the scopes cover different row counts");
    ORR_TRY(bind_device(lane));
    {
        Timed t(lane, "scope_combine", 12.0 * (double)dst->words);
        HIP_TRY(orr::launch_scope_combine(dst->bm, src->bm, dst->words, op, lane->stream));
    }
    const int r = refresh_scope(lane, dst);
    if (r != ORR_OK) (void)hipStreamSynchronize(lane->stream);
    return r;
}

// orr_scope_row_ids behind its locks: the ids of the scope's `live` rows (> 0) in candidate order into out_ids (host memory)
static int scope_row_ids_held(orr_index *lane, const orr_scope *s, int64_t live, int64_t *out_ids)
{
    ORR_TRY(bind_device(lane));
    hipStream_t st = lane->stream;
    // the bitmap compacted into entries in candidate order (the scoped pass's kernel, one pseudo-query), then their ids gathered
    const uint32_t ecap = scope::slice_cap((uint32_t)live);
    DevBuf entries, d_ids;
    auto body = [&]() -> int {
        ORR_TRY(entries.reserve(sizeof(orr::SelEntry) * (size_t)ecap));
        ORR_TRY(d_ids.reserve(sizeof(int64_t) * (size_t)live));
        ORR_TRY(lane->pin_scope.reserve(16));
        ORR_TRY(lane->ws_scope_meta.reserve(8));
        ORR_TRY(lane->ws_scope_sel.reserve(sizeof(uint32_t)));
        *lane->pin_scope.as<int64_t>() = live;
        HIP_TRY(hipMemcpyAsync(lane->ws_scope_meta.p, lane->pin_scope.p, 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(lane->ws_scope_sel.p, 0, sizeof(uint32_t), st));
        HIP_TRY(orr::launch_scope_compact(s->bm, s->words, 1, s->chunks, lane->ws_scope_sel.as<uint32_t>(), 1, lane->ws_scope_meta.as<int64_t>(),
                                          entries.as<orr::SelEntry>(), ecap, st));
        HIP_TRY(orr::launch_scope_entry_ids(entries.as<orr::SelEntry>(), live, lane->d_row_ids, lane->n_rows, d_ids.as<int64_t>(), st));
        HIP_TRY(hipMemcpyAsync(out_ids, d_ids.p, sizeof(int64_t) * (size_t)live, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ORR_OK;
    };
    const int r = body();
    if (r != ORR_OK) (void)hipStreamSynchronize(st);
    entries.release(); d_ids.release();
    return r;
}

// The fill of a cosine scope (orr_scope_near_plan.h), on the lane the caller holds:
//   1. no probes: the empty scope.  A foreign dim: every cosine is 0 -- all rows or none (scope_fill_range), no row is walked;
//   2. the probes brought to the device (they may live there already) and their exact norms taken as the queries' are
//      (launch_dot_exact, self_norm);
//   3. scope_near: launch_dot_exact's walk, a bit per row, every word written; pairs the device may not decide go to the band
//      list.  A list that was too short grows from the measured count and the walk runs again: never a truncated list;
//   4. the band: the listed rows' norms gathered, the list read back, every pair decided by scope_near::cosine_of on the HOST --
//      exact_score's expression -- and the pending rows that fold to false cleared (they were written set);
//   5. the deleted rows cleared.
// The search statistics do not move (this is no search); the kernel statistics record the launches.
static int scope_fill_near(orr_index *lane, orr_scope *sc, int32_t n_probes, int32_t dim, const float *probes, double min_cosine, int32_t mode)
{
    const orr_index *own = owner_of(lane);
    hipStream_t s = lane->stream;
    const int64_t n = lane->n_rows;
    if (n_probes == 0 || n <= 0) {                     // nothing to compare with: the empty scope
        HIP_TRY(hipMemsetAsync(sc->bm, 0, sizeof(uint32_t) * (size_t)sc->words, s));
        return ORR_OK;
    }
    if (scope_near::foreign_dim(dim, lane->dim)) {
        Timed t(lane, "scope_fill_range", 4.0 * (double)sc->words);
        HIP_TRY(orr::launch_scope_fill_range(sc->bm, sc->words, 0, scope_near::all_rows_at_zero(min_cosine) ? n : 0, s));
    } else {
        ORR_TRY(lane->ws_near_q.reserve(sizeof(float) * (size_t)n_probes * (size_t)dim));
        ORR_TRY(lane->ws_near_norm.reserve(sizeof(double) * (size_t)scope_near::kMaxProbes));
        ORR_TRY(lane->ws_near_cnt.reserve(sizeof(unsigned long long)));
        HIP_TRY(hipMemcpyAsync(lane->ws_near_q.p, probes, sizeof(float) * (size_t)n_probes * (size_t)dim, hipMemcpyDefault, s));
        {
            Timed t(lane, "scope_near_probe_norms", (4.0 * dim + 8.0) * n_probes);
            HIP_TRY(orr::launch_dot_exact(lane->ws_near_q.as<float>(), n_probes, dim, nullptr, 1, true, lane->ws_near_norm.as<double>(), n_probes, s));
        }
        unsigned long long count = 0;
        for (int attempt = 0;; ++attempt) {
            const int64_t cap = lane->near_band_cap;
            ORR_TRY(lane->ws_near_band.reserve(sizeof(scope_near::BandEntry) * (size_t)cap));
            HIP_TRY(hipMemsetAsync(lane->ws_near_cnt.p, 0, sizeof(unsigned long long), s));
            {
                Timed t(lane, "scope_near", 4.0 * (double)n * dim + 8.0 * (double)n + 4.0 * (double)sc->words);
                HIP_TRY(orr::launch_scope_near(lane->d_emb, n, dim, lane->ws_near_q.as<float>(), n_probes, lane->ws_near_norm.as<double>(), lane->d_norm_b,
                                               min_cosine, mode, lane->ws_near_band.as<scope_near::BandEntry>(),
                                               lane->ws_near_cnt.as<unsigned long long>(), cap, sc->bm, sc->words, s));
            }
            HIP_TRY(hipMemcpyAsync(&count, lane->ws_near_cnt.p, sizeof(count), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (count <= (unsigned long long)cap) break;
            if (count > (unsigned long long)scope_near::kMaxBandCap || attempt + 1 >= scope_near::kMaxWalks)
                return fail(ORR_EDEVICE, "orr_scope_create_near: the band list kept overflowing (%llu pairs)", count);
            lane->near_band_cap = scope_near::grown_cap((int64_t)count);
        }
        if (count > 0) {
            const size_t m = (size_t)count;
            ORR_TRY(lane->ws_near_rows.reserve(sizeof(double) * m));
            {
                Timed t(lane, "scope_near_band_norms", 32.0 * (double)m);
                HIP_TRY(orr::launch_scope_near_band_norms(lane->ws_near_band.as<scope_near::BandEntry>(), (int64_t)m, lane->d_norm_b, n, lane->ws_near_rows.as<double>(), s));
            }
            std::vector<scope_near::BandEntry> band(m);
            std::vector<double> norm_b(m);
            double norm_a[scope_near::kMaxProbes] = {};
            HIP_TRY(hipMemcpyAsync(band.data(), lane->ws_near_band.p, sizeof(scope_near::BandEntry) * m, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(norm_b.data(), lane->ws_near_rows.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(norm_a, lane->ws_near_norm.p, sizeof(double) * (size_t)n_probes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            std::vector<size_t> order(m);
            for (size_t i = 0; i < m; ++i) order[i] = i;
            std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return band[a].pos < band[b].pos; });
            std::vector<int64_t> out_rows;             // the pending rows the host decides OUT: their bits were written set
            for (size_t i = 0; i < m;) {
                double c[scope_near::kMaxProbes];
                int32_t k = 0;
                const uint32_t pos = band[order[i]].pos;
                for (; i < m && band[order[i]].pos == pos; ++i) {
                    const scope_near::BandEntry &e = band[order[i]];
                    if ((int64_t)pos >= n || e.probe >= (uint32_t)n_probes || k >= scope_near::kMaxProbes)
                        return fail(ORR_EDEVICE, "orr_scope_create_near: a malformed band entry (row %u, probe %u)", e.pos, e.probe);
                    c[k++] = scope_near::cosine_of(e.dot, norm_a[e.probe], norm_b[order[i]]);
                }
                if (!scope_near::pending_row_in(c, k, min_cosine, mode)) out_rows.push_back((int64_t)pos);
            }
            if (!out_rows.empty()) {                   // (ws_near_rows holds 8 bytes per band entry: enough for a position per row)
                HIP_TRY(hipMemcpyAsync(lane->ws_near_rows.p, out_rows.data(), sizeof(int64_t) * out_rows.size(), hipMemcpyHostToDevice, s));
                {
                    Timed t(lane, "scope_near_fixup", 12.0 * (double)out_rows.size());
                    HIP_TRY(orr::launch_scope_clear_positions(sc->bm, sc->words, lane->ws_near_rows.as<int64_t>(), (int64_t)out_rows.size(), s));
                }
                HIP_TRY(hipStreamSynchronize(s));      // out_rows is read until here
            }
            if (lane->profiling == 1) lane->stats[(size_t)stat_slot(lane, "scope_near_band_pairs")].algo_bytes += 16.0 * (double)m;
        }
    }
    Timed t(lane, "scope_clear_positions", 12.0 * (double)own->dead.size());
    HIP_TRY(orr::launch_scope_clear_positions(sc->bm, sc->words, own->d_dead.as<int64_t>(), (int64_t)own->dead.size(), s));
    return ORR_OK;
}

// the argument errors of orr_scope_create_near and its cluster form, in their order (scope_near::first_invalid)
static int near_arguments(const char *fn, bool out_null, int32_t n_probes, int32_t dim, const float *probes, int32_t mode, double min_cosine)
{
    switch (scope_near::first_invalid(out_null, n_probes, dim, probes == nullptr, mode, min_cosine)) {
    case 0: return ORR_OK;
    case 1: return fail(ORR_EINVAL, "%s: out is NULL", fn);
    case 2: return fail(ORR_EINVAL, "%s: n_probes must be in 0 .. %d (fold more with orr_scope_combine)", fn, scope_near::kMaxProbes);
    case 3: return fail(ORR_EINVAL, "%s: dim is negative", fn);
    case 4: return fail(ORR_EINVAL, "%s: probes is NULL with %d probes of dim %d", fn, n_probes, dim);
    case 5: return fail(ORR_EINVAL, "%s: mode must be ORR_NEAR_ALL (0) or ORR_NEAR_ANY (1)", fn);
    default: return fail(ORR_EINVAL, "%s: min_cosine is NaN", fn);
    }
}

int orr_scope_create_near(orr_index *idx, int32_t n_probes, int32_t dim, const float *probes, double min_cosine, int32_t mode, orr_scope **out)
{
    ORR_TRY(near_arguments("orr_scope_create_near", out == nullptr, n_probes, dim, probes, mode, min_cosine));
    if (!idx) return fail(ORR_EINVAL, "orr_scope_create_near: null index");
    return make_scope(idx, "orr_scope_create_near", out, [&](orr_index *lane, orr_scope *sc) -> int {
        return scope_fill_near(lane, sc, n_probes, dim, probes, min_cosine, mode);
    });
}

int orr_scope_add_ids(orr_scope *s, int64_t n_ids, const int64_t *ids, int64_t *out_added)
{
    if (n_ids < 0) return fail(ORR_EINVAL, "orr_scope_add_ids: n_ids is negative");
    if (n_ids > 0 && !ids) return fail(ORR_EINVAL, "orr_scope_add_ids: ids is NULL with %lld ids", (long long)n_ids);
    if (!s) return fail(ORR_EINVAL, "orr_scope_add_ids: null scope");
    orr_index *own = nullptr;
    ORR_TRY(scope_owner(s, nullptr, "orr_scope_add_ids", &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::unique_lock<std::shared_mutex> w(s->mu);
    ORR_TRY(scope_owner(s, nullptr, "orr_scope_add_ids", &own));
    return scope_add_ids_held(lane, s, n_ids, ids, out_added);
}

int orr_scope_combine(orr_scope *dst, int32_t op, const orr_scope *src)
{
    if (!scope_set::op_valid(op)) return fail(ORR_EINVAL, "orr_scope_combine: op must be ORR_SCOPE_AND (0), ORR_SCOPE_OR (1) or ORR_SCOPE_ANDNOT (2)");
    if (!dst || !src) return fail(ORR_EINVAL, "orr_scope_combine: null scope");
    orr_index *own = nullptr, *own_src = nullptr;
    ORR_TRY(scope_owner(dst, nullptr, "orr_scope_combine", &own));
    ORR_TRY(scope_owner(src, nullptr, "orr_scope_combine", &own_src));
    if (own != own_src) return fail(ORR_EINVAL, "orr_scope_combine: the scopes belong to different shards");
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    // dst exclusively, src shared, the lower address first (two combines with the roles swapped must not wait for each other)
    std::unique_lock<std::shared_mutex> w(dst->mu, std::defer_lock);
    std::shared_lock<std::shared_mutex> rd(src->mu, std::defer_lock);
    if (src == dst) w.lock();
    else if ((const void *)dst < (const void *)src) { w.lock(); rd.lock(); }
    else { rd.lock(); w.lock(); }
    ORR_TRY(scope_owner(dst, nullptr, "orr_scope_combine", &own));
    ORR_TRY(scope_owner(src, nullptr, "orr_scope_combine", &own_src));
    return scope_combine_held(lane, dst, op, src);
}

int64_t orr_scope_rows(const orr_scope *s)
{
    if (!s || !s->owner.load()) return -1;
    return s->live.load();
}

int orr_scope_row_ids(orr_scope *s, int64_t cap, int64_t *out_ids, int64_t *out_n)
{
    if (cap < 0) return fail(ORR_EINVAL, "orr_scope_row_ids: cap is negative");
    if (!out_n) return fail(ORR_EINVAL, "orr_scope_row_ids: out_n is NULL");
    if (cap > 0 && !out_ids) return fail(ORR_EINVAL, "orr_scope_row_ids: out_ids is NULL with room for %lld ids", (long long)cap);
    if (!s) return fail(ORR_EINVAL, "orr_scope_row_ids: null scope");
    orr_index *own = nullptr;
    ORR_TRY(scope_owner(s, nullptr, "orr_scope_row_ids", &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rd(s->mu);
    ORR_TRY(scope_owner(s, nullptr, "orr_scope_row_ids", &own));
    const int64_t live = s->live.load();
    *out_n = live;
    if (live > cap) return fail(ORR_EINVAL, "orr_scope_row_ids: the scope holds %lld rows, out_ids has room for %lld", (long long)live, (long long)cap);
    if (live == 0) return ORR_OK;
    return scope_row_ids_held(lane, s, live, out_ids);
}

void orr_scope_destroy(orr_scope *s)
{
    if (!s) return;
    std::lock_guard<std::mutex> life(g_scope_life_mu); // (the owning index is not destroyed meanwhile)
    orr_index *own = s->owner.load();
    if (own) {                                         // (the shard's maintenance holds scope_mu while it walks its scopes)
        std::lock_guard<std::mutex> g(own->scope_mu);
        own->scopes.erase(std::remove(own->scopes.begin(), own->scopes.end(), s), own->scopes.end());
    }
    {
        std::unique_lock<std::shared_mutex> w(s->mu);  // waits for the searches that hold it
        if (s->owner.load()) {
            (void)hipSetDevice(own->device);
            free_scope_arrays(s->bm, s->chunks);
        }
        s->bm = nullptr; s->chunks = nullptr;
    }
    delete s;
}

int orr_search_batch_in_scope(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                              const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                              int64_t candidate_limit, const orr_scope *scope, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    static const char *fn = "orr_search_batch_in_scope";
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    if (!scope) return fail(ORR_EINVAL, "%s: null scope", fn);
    ORR_TRY(check_batch(idx, a, fn));
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "%s: output buffers are required", fn);
    orr_index *own = nullptr;
    ORR_TRY(scope_owner(scope, idx, fn, &own));
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    std::shared_lock<std::shared_mutex> rd(scope->mu);
    ORR_TRY(scope_owner(scope, idx, fn, &own));
    if (scope->n_rows != idx->n_rows) return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)scope->n_rows, (long long)idx->n_rows);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return masked_batch(idx, a, ScopeSource{nullptr, scope}, out_rows, out_scores, out_counts);
}

int orr_search_batch_in_scopes(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                               const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                               int64_t candidate_limit, int32_t n_scopes, const orr_scope *const *scopes, const int32_t *query_scope,
                               int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    static const char *fn = "orr_search_batch_in_scopes";
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    if (!scope_set::scopes_valid(n_scopes)) return fail(ORR_EINVAL, "%s: n_scopes must be in 1 .. %d", fn, scope_set::kMaxScopes);
    if (!scopes) return fail(ORR_EINVAL, "%s: scopes is NULL", fn);
    if (!query_scope) return fail(ORR_EINVAL, "%s: query_scope is NULL", fn);
    if (B > 0 && !group::assignment_valid(query_scope, B, n_scopes))
        return fail(ORR_EINVAL, "%s: query_scope must name a scope in 0 .. %d for every query", fn, n_scopes - 1);
    for (int32_t g = 0; g < n_scopes; ++g)
        if (!scopes[g]) return fail(ORR_EINVAL, "%s: scopes[%d] is a null scope", fn, g);
    ORR_TRY(check_batch(idx, a, fn));
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "%s: output buffers are required", fn);
    orr_index *own = nullptr;
    for (int32_t g = 0; g < n_scopes; ++g) ORR_TRY(scope_owner(scopes[g], idx, fn, &own));
    Lane ln = acquire_lane(idx);
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    // every distinct scope shared, in address order
    std::vector<const orr_scope *> distinct(scopes, scopes + n_scopes);
    std::sort(distinct.begin(), distinct.end(), std::less<const orr_scope *>());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    std::vector<std::shared_lock<std::shared_mutex>> held;
    held.reserve(distinct.size());
    for (const orr_scope *sc : distinct) held.emplace_back(sc->mu);
    for (const orr_scope *sc : distinct) {
        ORR_TRY(scope_owner(sc, idx, fn, &own));
        if (sc->n_rows != idx->n_rows) return fail(ORR_ESTATE, "%s: a scope covers %lld rows, the handle %lld", fn, (long long)sc->n_rows, (long long)idx->n_rows);
    }
    GroupArgs ga{n_scopes, 0, nullptr, nullptr, query_scope};
    ga.scopes = scopes;
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return grouped_batch(idx, a, ga, out_rows, out_scores, out_counts);
}

// ---- cosine range search (orr_search_range_cosine; the rules are orr_range_plan.h's) ----------------------------------------

struct RangeArgs {
    int32_t B, dim;
    const float *q;
    const double *min_cosine;
    int32_t max_hits;
    bool bulk = false;                                 // orr_search_range_cosine_bulk: up to range_bulk::kMaxQueries queries, the GEMM screen where its rules send them
    const char *fn = "orr_search_range_cosine";
};

// One shard's answer: per query its best max_hits hits in order and the exact number of hits -- or, with `limit`, no hits
// and in `total` the pairs each query's screen kept (an upper bound of its hits).
struct RangeOut {
    std::vector<std::vector<range::Hit>> hits;
    std::vector<int64_t> total;
    bool limit = false;
};

// The host's decision of one query's list: cosine_of and >= on every pair it received, the order, the cut.
static void range_finish_query(const std::vector<range::ListEntry> &list, double norm_a, double t, int32_t max_hits, int64_t row_base,
                               std::vector<range::Hit> &hits, int64_t &total)
{
    struct Scored { double c; uint32_t pos; int64_t row_id; };
    std::vector<Scored> kept;
    for (const range::ListEntry &e : list) {
        const double c = scope_near::cosine_of(e.dot, norm_a, e.norm_b);
        if (scope_near::verdict(c, t)) kept.push_back(Scored{c, e.pos, e.row_id});
    }
    total = (int64_t)kept.size();
    const size_t take = (size_t)std::min<int64_t>(total, max_hits);
    auto first = [](const Scored &a, const Scored &b) { return range::before(a.c, (int64_t)a.pos, b.c, (int64_t)b.pos); };
    std::partial_sort(kept.begin(), kept.begin() + (ptrdiff_t)take, kept.end(), first);
    hits.clear();
    hits.reserve(take);
    for (size_t i = 0; i < take; ++i) hits.push_back(range::Hit{kept[i].row_id, row_base + (int64_t)kept[i].pos, kept[i].c});
}

// What one call carries from stage to stage (range_run lists the stages): the lane and the call, the allowed rows, the queries'
// norms, the walk plan (range_bulk::walk_of), what the kernels read per walked query, and the pair counters.
struct RangeWork {
    orr_index *const lane;
    const RangeArgs &a;
    RangeOut &o;
    const hipStream_t s;
    const int32_t B, D;
    const int64_t n, words, allowed_rows;
    const uint32_t *allowed = nullptr;                 // the scope's bitmap, or ws_range_allowed
    std::vector<double> norm_a, err2;                  // per query: the exact norm; the two-level quantisation error (+inf: none was taken)
    bool shadow = false;                               // the int8 shadow is in place, and the screen may read it
    range_bulk::Walk walk;
    int32_t ns = 0, nw = 0;                            // walk.n_screen; the walked queries, walk.perm.size()
    // per walked query, in walk.perm's order
    const float *Qp = nullptr;
    const int8_t *q1 = nullptr, *q2 = nullptr;         // the SCREEN queries' two int8 levels
    const double *d_err1 = nullptr;                    // ... and their one-level error (the GEMM's)
    double *d_na = nullptr, *d_t = nullptr;
    orr::QueryConst *d_qc = nullptr;
    uint32_t *d_cnt = nullptr, *d_lcnt = nullptr;
    // A query's kept pairs exceeded "range_pair_cap": from here on the call only counts -- nothing is stored, re-scored or read
    // back, and o.total receives the counters.  It becomes o.limit.
    bool counting = false;
    double screen_pairs = 0.0, host_pairs = 0.0;
    std::vector<uint32_t> h_cnt, h_lcnt;               // a launch group's counters on the host
    std::vector<range::ListEntry> list;

    RangeWork(orr_index *l, const RangeArgs &args, const orr_scope *within, RangeOut &out)
        : lane(l), a(args), o(out), s(l->stream), B(args.B), D(l->dim), n(l->n_rows), words(keyword::words_per_term(l->n_rows)),
          allowed_rows(within ? within->live.load() : l->n_rows - (int64_t)owner_of(l)->dead.size()) {}

    // entries per query: the sticky size as the screen uses it (its launch groups are sized by it) ...
    int64_t buffer_cap() const { return range::buffer_cap(lane->range_buffer); }
    // ... what the survivors' buffers hold, and what the exact form's lists hold: one entry each in a call that only counts
    int64_t buffer_entries() const { return counting ? 1 : buffer_cap(); }
    int64_t list_entries() const { return counting ? 1 : range::buffer_cap(std::max(lane->range_buffer, lane->range_list_cap), range::kMaxPairCap); }
};

static void range_stat(orr_index *lane, const char *name, double v)
{
    if (lane->profiling == 1) lane->stats[(size_t)stat_slot(lane, name)].algo_bytes += v;
}

// 1. the allowed rows: the scope's bitmap, or all rows with the deleted ones cleared
static int range_allowed_rows(RangeWork &w, const orr_scope *within)
{
    orr_index *lane = w.lane;
    if (within) {
        if (within->words != w.words)
            return fail(ORR_ESTATE, "%s: the scope's bitmap has %lld words, the shard's %lld", w.a.fn, (long long)within->words, (long long)w.words);
        w.allowed = within->bm;
        return ORR_OK;
    }
    const orr_index *own = owner_of(lane);
    ORR_TRY(lane->ws_range_allowed.reserve(sizeof(uint32_t) * (size_t)w.words));
    {
        Timed t(lane, "scope_fill_range", 4.0 * (double)w.words);
        HIP_TRY(orr::launch_scope_fill_range(lane->ws_range_allowed.as<uint32_t>(), w.words, 0, w.n, w.s));
    }
    Timed t(lane, "scope_clear_positions", 12.0 * (double)own->dead.size());
    HIP_TRY(orr::launch_scope_clear_positions(lane->ws_range_allowed.as<uint32_t>(), w.words, own->d_dead.as<int64_t>(), (int64_t)own->dead.size(), w.s));
    w.allowed = lane->ws_range_allowed.as<uint32_t>();
    return ORR_OK;
}

// 2. the queries brought to the device (they may live there already), their exact norms taken as a search takes them, and -- where
// the screen's shape holds and the int8 shadow is in place -- their int8 images with the quantisation errors.  A foreign dim
// reads no query: every one is AT ZERO.
static int range_queries(RangeWork &w)
{
    orr_index *lane = w.lane;
    const int32_t B = w.B, D = w.D;
    hipStream_t s = w.s;
    w.norm_a.assign((size_t)B, 0.0);
    w.err2.assign((size_t)B, std::numeric_limits<double>::infinity());
    if (scope_near::foreign_dim(w.a.dim, D)) return ORR_OK;
    ORR_TRY(lane->ws_range_q.reserve(sizeof(float) * (size_t)B * (size_t)D));
    ORR_TRY(lane->ws_range_norm.reserve(sizeof(double) * (size_t)B));
    HIP_TRY(hipMemcpyAsync(lane->ws_range_q.p, w.a.q, sizeof(float) * (size_t)B * (size_t)D, hipMemcpyDefault, s));
    {
        Timed t(lane, "range_query_norms", (4.0 * D + 8.0) * B);
        HIP_TRY(orr::launch_dot_exact(lane->ws_range_q.as<float>(), B, D, nullptr, 1, true, lane->ws_range_norm.as<double>(), B, s));
    }
    HIP_TRY(hipMemcpyAsync(w.norm_a.data(), lane->ws_range_norm.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, s));
    if (lane->opt_range_form != range::Exact && range_bulk::stream_shape(D)) {
        ORR_TRY(ensure_i8_shadow(lane));               // directly: the screen runs on a shard of any size
        if (lane->is_view && !lane->i8_ready && lane->parent) {
            // a lane made before its index had the shadow borrows it now -- when the index's own lane is idle; else the
            // exact form answers this call (the shadow is only dropped with every lane idle: insert, compact)
            orr_index *p = const_cast<orr_index *>(lane->parent);
            if (p->mu.try_lock()) {
                if (p->i8_ready) borrow_shadows(p, lane);
                p->mu.unlock();
            }
        }
        w.shadow = lane->i8_ready;
    }
    if (w.shadow) {
        ORR_TRY(lane->ws_q8.reserve(2 * (size_t)B * (size_t)D));
        ORR_TRY(lane->ws_q8s1.reserve(sizeof(float) * (size_t)B));
        ORR_TRY(lane->ws_q8err.reserve(2 * sizeof(double) * (size_t)B));
        {
            Timed t(lane, "range_i8_queries", 6.0 * (double)B * D);
            HIP_TRY(orr::launch_i8_queries(lane->ws_range_q.as<float>(), B, D, lane->ws_q8.p, lane->ws_q8s1.as<float>(), lane->ws_q8err.as<double>(), s,
                                           lane->ws_q8err.as<double>() + B));
        }
        HIP_TRY(hipMemcpyAsync(w.err2.data(), lane->ws_q8err.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return ORR_OK;
}

// 3a. the queries AT ZERO: every allowed row, in candidate order, with cosine 0 -- or none.  The rows are listed once.
static int range_answers_at_zero(RangeWork &w)
{
    orr_index *lane = w.lane;
    hipStream_t s = w.s;
    bool any = false;
    for (int32_t b : w.walk.zero) {
        if (!scope_near::all_rows_at_zero(w.a.min_cosine[b])) continue;
        w.o.total[(size_t)b] = w.allowed_rows;
        any = true;
    }
    if (!any || w.a.max_hits == 0) return ORR_OK;
    const size_t take = (size_t)std::min<int64_t>(w.allowed_rows, w.a.max_hits);
    std::vector<uint32_t> bm((size_t)w.words);
    HIP_TRY(hipMemcpyAsync(bm.data(), w.allowed, sizeof(uint32_t) * (size_t)w.words, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<orr::SelEntry> ent;
    ent.reserve(take);
    for (int64_t r = 0; r < w.n && ent.size() < take; ++r)
        if ((bm[(size_t)(r >> 5)] >> (uint32_t)(r & 31)) & 1u) { orr::SelEntry e; e.key = 0; e.pos = (uint32_t)r; e.pad = 0; ent.push_back(e); }
    std::vector<int64_t> ids(ent.size());
    if (!ent.empty()) {
        ORR_TRY(lane->ws_range_buf.reserve(sizeof(orr::SelEntry) * ent.size()));
        ORR_TRY(lane->ws_range_bdot.reserve(sizeof(int64_t) * ent.size()));
        HIP_TRY(hipMemcpyAsync(lane->ws_range_buf.p, ent.data(), sizeof(orr::SelEntry) * ent.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(orr::launch_scope_entry_ids(lane->ws_range_buf.as<orr::SelEntry>(), (int64_t)ent.size(), lane->d_row_ids, w.n, lane->ws_range_bdot.as<int64_t>(), s));
        HIP_TRY(hipMemcpyAsync(ids.data(), lane->ws_range_bdot.p, sizeof(int64_t) * ent.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    std::vector<range::Hit> zero_hits;
    for (size_t i = 0; i < ent.size(); ++i) zero_hits.push_back(range::Hit{ids[i], lane->row_base + (int64_t)ent[i].pos, 0.0});
    for (int32_t b : w.walk.zero)
        if (scope_near::all_rows_at_zero(w.a.min_cosine[b])) w.o.hits[(size_t)b] = zero_hits;
    return ORR_OK;
}

// 3b. the walked queries in walk.perm's order, with what the kernels read per query.  TWO LAYOUTS: a batch that is in that order
// already (walk.in_place) is used where it lies -- Qp is the batch and the int8 image is range_queries' of all B queries; any
// other batch is copied into the order, and its ns SCREEN queries, now in front, are imaged again.  launch_i8_queries puts the
// second level behind the first of the batch it was given: behind B queries in the one layout, behind ns in the other.  The
// one-level errors stay behind the B two-level ones either way.
static int range_stage_walked(RangeWork &w)
{
    orr_index *lane = w.lane;
    const int32_t B = w.B, D = w.D, ns = w.ns, nw = w.nw;
    const std::vector<int32_t> &perm = w.walk.perm;
    hipStream_t s = w.s;
    w.Qp = lane->ws_range_q.as<float>();
    if (!w.walk.in_place) {
        ORR_TRY(lane->ws_range_qp.reserve(sizeof(float) * (size_t)nw * (size_t)D));
        for (int32_t p = 0; p < nw; ++p)
            HIP_TRY(hipMemcpyAsync(lane->ws_range_qp.as<float>() + (size_t)p * D, lane->ws_range_q.as<float>() + (size_t)perm[(size_t)p] * D,
                                   sizeof(float) * (size_t)D, hipMemcpyDeviceToDevice, s));
        w.Qp = lane->ws_range_qp.as<float>();
        if (ns > 0) {
            Timed t(lane, "range_i8_queries", 6.0 * (double)ns * D);
            HIP_TRY(orr::launch_i8_queries(w.Qp, ns, D, lane->ws_q8.p, lane->ws_q8s1.as<float>(), lane->ws_q8err.as<double>(), s, lane->ws_q8err.as<double>() + B));
        }
    }
    if (ns > 0) {
        w.q1 = static_cast<const int8_t *>(lane->ws_q8.p);
        w.q2 = w.q1 + (size_t)(w.walk.in_place ? B : ns) * (size_t)D;
        w.d_err1 = lane->ws_q8err.as<double>() + B;
    }
    std::vector<double> h_na((size_t)nw), h_t((size_t)nw);
    std::vector<orr::QueryConst> h_qc((size_t)nw);
    for (int32_t p = 0; p < nw; ++p) {
        const int32_t b = perm[(size_t)p];
        h_na[(size_t)p] = w.norm_a[(size_t)b];
        h_t[(size_t)p] = w.a.min_cosine[b];
        orr::QueryConst qc{};
        qc.norm_a = w.norm_a[(size_t)b];
        qc.inv_sqrt_na = 1.0 / std::sqrt(w.norm_a[(size_t)b]);
        qc.use_cos = 1;
        h_qc[(size_t)p] = qc;
    }
    ORR_TRY(lane->ws_range_consts.reserve((2 * sizeof(double) + sizeof(orr::QueryConst)) * (size_t)nw));
    w.d_na = lane->ws_range_consts.as<double>();
    w.d_t = w.d_na + nw;
    w.d_qc = reinterpret_cast<orr::QueryConst *>(w.d_t + nw);
    HIP_TRY(hipMemcpyAsync(w.d_na, h_na.data(), sizeof(double) * (size_t)nw, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.d_t, h_t.data(), sizeof(double) * (size_t)nw, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.d_qc, h_qc.data(), sizeof(orr::QueryConst) * (size_t)nw, hipMemcpyHostToDevice, s));
    ORR_TRY(lane->ws_range_cnt.reserve(sizeof(uint32_t) * 2 * (size_t)nw));
    w.d_cnt = lane->ws_range_cnt.as<uint32_t>();
    w.d_lcnt = w.d_cnt + nw;
    // the GEMM reads the tiled image of the SCREEN queries' first int8 level
    if (w.walk.gemm) {
        ORR_TRY(lane->ws_qtiled.reserve(orr::i8_tiled_bytes(ns, D)));
        ORR_TRY(lane->ws_tickets.reserve(sizeof(uint32_t) * 8 * 16));
        ORR_TRY(lane->ws_range_args.reserve(orr::kRangeTile16ArgsBytes));
        Timed t(lane, "range_i8_tile_queries", 2.0 * (double)ns * D);
        HIP_TRY(orr::launch_i8_tile_queries(w.q1, ns, D, lane->ws_qtiled.p, s));
    }
    return ORR_OK;
}

// THE GROWTH RULE, the screen's buffers' and the exact form's lists' alike.  `count`: what nq queries wanted of `cap` entries each.
enum class RangeFit {
    Fits,                                              // go on: everything was stored
    CountOnly,                                         // a query exceeded "range_pair_cap": the call only counts from now on
    Again,                                             // too short: `sticky` has grown from the measured count (the lane keeps it), run again
    Full,                                              // too short, and the caller allows no growth
};
static RangeFit range_fit(RangeWork &w, const uint32_t *count, int32_t nq, int64_t cap, bool may_grow, int64_t &sticky, int64_t max_cap, uint32_t &worst)
{
    worst = *std::max_element(count, count + nq);
    if ((int64_t)worst > w.lane->opt_range_pair_cap) w.counting = true;
    if (w.counting) return RangeFit::CountOnly;
    if ((int64_t)worst <= cap) return RangeFit::Fits;
    if (!may_grow) return RangeFit::Full;
    sticky = range::grown_cap((int64_t)worst, max_cap);
    range_stat(w.lane, "range_buffer_growths", 1.0);
    return RangeFit::Again;
}

// ... and what a call that only counts leaves of the walked queries [p0, p0 + nq): the counters, upper bounds of their hits
static void range_totals_are_counts(RangeWork &w, int32_t p0, int32_t nq, const uint32_t *count)
{
    for (int32_t i = 0; i < nq; ++i) w.o.total[(size_t)w.walk.perm[(size_t)(p0 + i)]] = (int64_t)count[i];
}

// 6. the lists of the walked queries [p0, p0 + nq) (lcap entries each, counts h_lcnt) read back, and every listed pair decided by
// the host (range_finish_query)
static int range_read_back(RangeWork &w, int32_t p0, int32_t nq, uint32_t lcap, const uint32_t *h_lcnt)
{
    orr_index *lane = w.lane;
    for (int32_t i = 0; i < nq; ++i) {
        const int32_t b = w.walk.perm[(size_t)(p0 + i)];
        w.list.resize(h_lcnt[i]);
        if (!w.list.empty()) {
            HIP_TRY(hipMemcpyAsync(w.list.data(), lane->ws_range_list.as<range::ListEntry>() + (size_t)i * lcap, sizeof(range::ListEntry) * w.list.size(), hipMemcpyDeviceToHost, w.s));
            HIP_TRY(hipStreamSynchronize(w.s));
        }
        w.host_pairs += (double)w.list.size();
        range_finish_query(w.list, w.norm_a[(size_t)b], w.a.min_cosine[b], w.a.max_hits, lane->row_base, w.o.hits[(size_t)b], w.o.total[(size_t)b]);
    }
    return ORR_OK;
}

// 5. one walk of the exact form, the walked queries [e0, e0 + nq), nq <= kMaxExactQ: launch_dot_exact over all rows ->
// range_collect_dense -> one list per query.  A list that was too short grows, and only the ending runs again: the dots stand.
static int range_exact_walk(RangeWork &w, int32_t e0, int32_t nq)
{
    orr_index *lane = w.lane;
    const int64_t n = w.n;
    hipStream_t s = w.s;
    ORR_TRY(lane->ws_range_dots.reserve(sizeof(double) * (size_t)nq * (size_t)n));
    {
        Timed t(lane, "range_dot_exact", 4.0 * (double)n * w.D + 8.0 * (double)nq * (double)n);
        HIP_TRY(orr::launch_dot_exact(lane->d_emb, n, w.D, w.Qp + (size_t)e0 * w.D, nq, false, lane->ws_range_dots.as<double>(), n, s));
    }
    uint32_t h_lcnt[orr::kMaxExactQ] = {}, mx = 0;
    int64_t lcap = 0;
    RangeFit fit = RangeFit::Again;
    for (int attempt = 0; fit == RangeFit::Again; ++attempt) {
        lcap = w.list_entries();
        ORR_TRY(lane->ws_range_list.reserve(sizeof(range::ListEntry) * (size_t)nq * (size_t)lcap));
        HIP_TRY(hipMemsetAsync(w.d_lcnt, 0, sizeof(uint32_t) * (size_t)nq, s));
        {
            Timed t(lane, "range_collect_dense", 8.0 * (double)nq * (double)n + 16.0 * (double)n);
            HIP_TRY(orr::launch_range_collect_dense(lane->ws_range_dots.as<double>(), n, nq, w.d_na + e0, lane->d_norm_b, lane->d_row_ids, n, w.allowed, w.d_t + e0,
                                                    lane->ws_range_list.as<range::ListEntry>(), w.d_lcnt, (uint32_t)lcap, s));
        }
        HIP_TRY(hipMemcpyAsync(h_lcnt, w.d_lcnt, sizeof(uint32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        fit = range_fit(w, h_lcnt, nq, lcap, attempt < 3, lane->range_list_cap, range::kMaxPairCap, mx);
        if (fit == RangeFit::Full) return fail(ORR_EDEVICE, "%s: a hit list kept overflowing (%u pairs)", w.a.fn, mx);
    }
    if (fit == RangeFit::CountOnly) { range_totals_are_counts(w, e0, nq, h_lcnt); return ORR_OK; }
    return range_read_back(w, e0, nq, (uint32_t)lcap, h_lcnt);
}

// ... over the walked queries [p0, p0 + cnt_q), kMaxExactQ per walk
static int range_exact_form(RangeWork &w, int32_t p0, int32_t cnt_q)
{
    for (int32_t e0 = p0; e0 < p0 + cnt_q; e0 += orr::kMaxExactQ) ORR_TRY(range_exact_walk(w, e0, std::min<int32_t>(orr::kMaxExactQ, p0 + cnt_q - e0)));
    return ORR_OK;
}

// 4a. one launch group of the screen, the walked SCREEN queries [b0, b0 + nq) at `cap` entries each: the GEMM in ONE launch, or
// the stream, kScreenQ queries per launch -> the survivors' buffers, their counters in w.h_cnt
static int range_screen_group(RangeWork &w, int32_t b0, int32_t nq, int64_t cap)
{
    orr_index *lane = w.lane;
    const int32_t D = w.D;
    const int64_t n = w.n;
    hipStream_t s = w.s;
    static_assert(range_bulk::kPairBytes == (int64_t)(sizeof(orr::SelEntry) + sizeof(double) + sizeof(range::ListEntry)), "what one kept pair takes");
    const uint32_t scap = (uint32_t)w.buffer_entries();
    ORR_TRY(lane->ws_range_buf.reserve(sizeof(orr::SelEntry) * (size_t)nq * (size_t)scap));
    if (!w.counting) {                                 // (what the re-score and the collecting write)
        ORR_TRY(lane->ws_range_bdot.reserve(sizeof(double) * (size_t)nq * (size_t)cap));
        ORR_TRY(lane->ws_range_list.reserve(sizeof(range::ListEntry) * (size_t)nq * (size_t)cap));
    }
    HIP_TRY(hipMemsetAsync(w.d_cnt, 0, sizeof(uint32_t) * 2 * (size_t)w.nw, s));
    if (w.walk.gemm) {
        // one launch for the group; queries [b0, b0 + nq) of the tiled image start at a query tile only for b0 == 0, so a
        // later group gets an image of its own
        if (b0 > 0) {
            Timed t(lane, "range_i8_tile_queries", 2.0 * (double)nq * D);
            HIP_TRY(orr::launch_i8_tile_queries(w.q1 + (size_t)b0 * D, nq, D, lane->ws_qtiled.p, s));
        }
        HIP_TRY(hipMemsetAsync(lane->ws_tickets.p, 0, sizeof(uint32_t) * 8, s));
        Timed t(lane, "screen_tile16_range", 1.0 * (double)n * D + 24.0 * (double)n + (double)orr::i8_tiled_bytes(nq, D));   // per row: scale, two relative norms, normB, its share of the bitmap
        HIP_TRY(orr::launch_screen_tile16_range(lane->ws_qtiled.p, lane->ws_q8s1.as<float>() + b0, w.d_err1 + b0, nq, lane->emb_i8.p, lane->i8_scale.as<float>(),
                                                lane->i8_rel_err.as<float>(), lane->i8_rel_hat.as<float>(), lane->d_norm_b, n, D, w.d_qc + b0, w.d_t + b0, w.allowed,
                                                w.d_cnt, lane->ws_range_buf.as<orr::SelEntry>(), scap, lane->ws_tickets.as<uint32_t>(), lane->ws_range_args.p, s));
    }
    for (int32_t g0 = 0; !w.walk.gemm && g0 < nq; g0 += range::kScreenQ) {
        const int32_t gq = std::min<int32_t>(range::kScreenQ, nq - g0), p = b0 + g0;
        Timed t(lane, "screen_gemv_i8_range", 1.0 * (double)n * D + 20.0 * (double)n + 2.0 * (double)gq * D);   // per row: scale, two relative norms, normB
        HIP_TRY(orr::launch_screen_gemv_i8_range(w.q1 + (size_t)p * D, w.q2 + (size_t)p * D, lane->ws_q8s1.as<float>() + p, lane->ws_q8err.as<double>() + p, gq,
                                                 lane->emb_i8.p, lane->i8_scale.as<float>(), lane->i8_rel_err.as<float>(), lane->i8_rel_hat.as<float>(),
                                                 lane->d_norm_b, n, D, w.d_qc + p, w.d_t + p, w.allowed, w.d_cnt + g0,
                                                 lane->ws_range_buf.as<orr::SelEntry>() + (size_t)g0 * scap, scap, s));
    }
    w.h_cnt.assign((size_t)nq, 0u);
    HIP_TRY(hipMemcpyAsync(w.h_cnt.data(), w.d_cnt, sizeof(uint32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ORR_OK;
}

// 4b. ... whose survivors, at most mx per query, fit: launch_rescore_buffer_exact -> range_collect -> one list per query -> the host
static int range_rescore_collect(RangeWork &w, int32_t b0, int32_t nq, int64_t cap, uint32_t mx)
{
    orr_index *lane = w.lane;
    hipStream_t s = w.s;
    for (int32_t i = 0; i < nq; ++i) w.screen_pairs += (double)w.h_cnt[(size_t)i];
    {
        Timed t(lane, "range_rescore_exact", (4.0 * w.D + 40.0) * (double)mx * nq);
        HIP_TRY(orr::launch_rescore_buffer_exact(lane->d_emb, w.D, w.Qp + (size_t)b0 * w.D, nq, lane->d_norm_b, lane->d_created, orr::KwView{}, w.d_qc + b0, 0, w.d_cnt,
                                                 (uint32_t)cap, lane->ws_range_buf.as<orr::SelEntry>(), lane->ws_range_bdot.as<double>(), s));
    }
    {
        Timed t(lane, "range_collect", 64.0 * (double)mx * nq);
        HIP_TRY(orr::launch_range_collect(lane->ws_range_buf.as<orr::SelEntry>(), lane->ws_range_bdot.as<double>(), w.d_cnt, (uint32_t)cap, nq, w.d_na + b0, lane->d_norm_b,
                                          lane->d_row_ids, w.n, w.d_t + b0, lane->ws_range_list.as<range::ListEntry>(), w.d_lcnt, (uint32_t)cap, s));
    }
    w.h_lcnt.assign((size_t)nq, 0u);
    HIP_TRY(hipMemcpyAsync(w.h_lcnt.data(), w.d_lcnt, sizeof(uint32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return range_read_back(w, b0, nq, (uint32_t)cap, w.h_lcnt.data());
}

// 4. the screen over the walked queries [0, ns): as many queries per launch group as their buffers allow
// (range_bulk::group_queries); a group whose buffers were too short runs again with the grown size
static int range_screen(RangeWork &w)
{
    for (int32_t b0 = 0, nq = 0; b0 < w.ns; b0 += nq) {
        int64_t cap = 0;
        uint32_t mx = 0;
        RangeFit fit = RangeFit::Again;
        while (fit == RangeFit::Again) {
            cap = w.buffer_cap();
            nq = std::min<int32_t>(w.ns - b0, range_bulk::group_queries(cap, w.walk.gemm ? 1 : range::kScreenQ));
            ORR_TRY(range_screen_group(w, b0, nq, cap));
            fit = range_fit(w, w.h_cnt.data(), nq, cap, cap < range::kMaxBuffer, w.lane->range_buffer, range::kMaxBuffer, mx);
        }
        if (fit == RangeFit::CountOnly) range_totals_are_counts(w, b0, nq, w.h_cnt.data());
        else if (fit == RangeFit::Full) ORR_TRY(range_exact_form(w, b0, nq));      // more survivors than a buffer of the exact re-score holds
        else ORR_TRY(range_rescore_collect(w, b0, nq, cap, mx));
    }
    return ORR_OK;
}

// The call on the lane the caller holds (with the scope, if any, held shared), stage by stage:
//   1. range_allowed_rows;
//   2. range_queries;
//   3. every query gets its form -- range_bulk::walk_of: AT ZERO (a foreign dim, a norm <= 0: every cosine is 0, no row is
//      walked), the SCREEN (stream_applies) or the EXACT form, and which screen (gemm_takes) -- and the walked queries their
//      order: range_answers_at_zero, range_stage_walked;
//   4. range_screen: range_screen_group -- the stream, K2i with the RANGE ending, or the int8 screening GEMM with the RANGE
//      ending, one launch per group -- -> range_rescore_collect; beyond range::kMaxBuffer survivors the exact form;
//   5. range_exact_form, kMaxExactQ queries per range_exact_walk;
//   6. range_read_back: the host decides every listed pair (range_finish_query).
// A buffer or list that was too short grows and its launches run again; a query whose kept pairs exceed "range_pair_cap" turns
// the call into counting (range_fit, RangeWork::counting): o.limit.  The search statistics do not move.
static int range_run(orr_index *lane, const RangeArgs &a, const orr_scope *within, RangeOut &o)
{
    RangeWork w(lane, a, within, o);
    o.hits.assign((size_t)w.B, {});
    o.total.assign((size_t)w.B, 0);
    o.limit = false;
    if (w.n <= 0 || w.allowed_rows <= 0) return ORR_OK;
    ORR_TRY(range_allowed_rows(w, within));
    ORR_TRY(range_queries(w));
    w.walk = range_bulk::walk_of(w.B, a.dim, w.D, w.norm_a.data(), w.err2.data(), w.shadow, lane->opt_range_form, lane->opt_range_gemm, a.bulk);
    w.ns = w.walk.n_screen;
    w.nw = (int32_t)w.walk.perm.size();
    ORR_TRY(range_answers_at_zero(w));
    if (w.nw == 0) return ORR_OK;
    ORR_TRY(range_stage_walked(w));
    ORR_TRY(range_screen(w));
    ORR_TRY(range_exact_form(w, w.ns, w.nw - w.ns));
    o.limit = w.counting;
    if (o.limit)                                       // the queries answered before the limit was met: their hits are an upper bound too
        for (int32_t b = 0; b < w.B; ++b) o.hits[(size_t)b].clear();
    range_stat(lane, "range_screen_pairs", 16.0 * w.screen_pairs);
    range_stat(lane, "range_host_pairs", 32.0 * w.host_pairs);
    return ORR_OK;
}

// ... and whatever it left on the stream is done before the caller's buffers go away
static int range_on_lane(orr_index *lane, const RangeArgs &a, const orr_scope *within, RangeOut &o)
{
    int r = bind_device(lane);
    if (r == ORR_OK) r = range_run(lane, a, within, o);
    if (r != ORR_OK) (void)hipStreamSynchronize(lane->stream);
    collect_events(lane);
    return r;
}

// the argument errors of orr_search_range_cosine and its cluster form, in their order (range::first_invalid)
static int range_arguments(const char *fn, const RangeArgs &a, const void *out_hits, const void *out_n, const void *out_total)
{
    int32_t bad = 0;
    const int32_t rule = a.bulk ? range_bulk::first_invalid(a.B, a.dim, a.q == nullptr, a.min_cosine, a.max_hits, out_hits == nullptr, out_n == nullptr, out_total == nullptr, &bad)
                                : range::first_invalid(a.B, a.dim, a.q == nullptr, a.min_cosine, a.max_hits, out_hits == nullptr, out_n == nullptr, out_total == nullptr, &bad);
    switch (rule) {
    case 0: return ORR_OK;
    case 1: return fail(ORR_EINVAL, "%s: the batch size must be in 0 .. %d", fn, a.bulk ? range_bulk::kMaxQueries : range::kMaxQueries);
    case 2: return fail(ORR_EINVAL, "%s: dim is negative", fn);
    case 3: return fail(ORR_EINVAL, "%s: max_hits is negative", fn);
    case 4: return fail(ORR_EINVAL, "%s: q is NULL with dim %d", fn, a.dim);
    case 5: return fail(ORR_EINVAL, "%s: min_cosine is NULL", fn);
    case 6: return fail(ORR_EINVAL, "%s: out_hits is NULL with max_hits %d", fn, a.max_hits);
    case 7: return fail(ORR_EINVAL, "%s: out_n is NULL", fn);
    case 8: return fail(ORR_EINVAL, "%s: out_total is NULL", fn);
    default: return fail(ORR_EINVAL, "%s: min_cosine[%d] is NaN", fn, bad);
    }
}

// The outputs of a call from its (merged) answer.  With the limit met: no hits, and the upper bounds in out_total.
static int range_write(const char *fn, const RangeArgs &a, const RangeOut &o, orr_range_hit *out_hits, int32_t *out_n, int64_t *out_total)
{
    for (int32_t b = 0; b < a.B; ++b) {
        out_total[b] = o.total[(size_t)b];
        out_n[b] = o.limit ? 0 : (int32_t)o.hits[(size_t)b].size();
        for (size_t i = 0; !o.limit && i < o.hits[(size_t)b].size(); ++i) {
            const range::Hit &h = o.hits[(size_t)b][i];
            out_hits[(size_t)b * (size_t)a.max_hits + i] = orr_range_hit{h.row_id, h.order_key, h.cosine};
        }
    }
    if (!o.limit) return ORR_OK;
    int32_t worst = 0;
    for (int32_t b = 1; b < a.B; ++b) if (o.total[(size_t)b] > o.total[(size_t)worst]) worst = b;
    return fail(ORR_ELIMIT, "%s: query %d keeps %lld pairs for the exact re-score, more than range_pair_cap: tighten its min_cosine (out_total holds every query's count), "
                            "or make a set with orr_scope_create_near", fn, worst, (long long)o.total[(size_t)worst]);
}

// orr_search_range_cosine and orr_search_range_cosine_bulk: one body, a.bulk apart
static int range_search(orr_index *idx, const RangeArgs &a, const orr_scope *within, orr_range_hit *out_hits, int32_t *out_n, int64_t *out_total)
{
    const char *fn = a.fn;
    ORR_TRY(range_arguments(fn, a, out_hits, out_n, out_total));
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    if (a.B == 0) return ORR_OK;
    orr_index *own = nullptr;
    if (within) ORR_TRY(scope_owner(within, idx, fn, &own));
    Lane ln = acquire_lane(idx);                       // like a search: its own lane, concurrent with the others
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rd;
    if (within) rd = std::shared_lock<std::shared_mutex>(within->mu);
    if (!lane->sealed) return fail(ORR_ESTATE, "%s: the index is not sealed", fn);
    if (within) {
        ORR_TRY(scope_owner(within, idx, fn, &own));
        if (within->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)within->n_rows, (long long)lane->n_rows);
    }
    RangeOut o;
    ORR_TRY(range_on_lane(lane, a, within, o));
    return range_write(fn, a, o, out_hits, out_n, out_total);
}

int orr_search_range_cosine(orr_index *idx, int32_t B, int32_t dim, const float *q, const double *min_cosine, const orr_scope *within,
                            int32_t max_hits, orr_range_hit *out_hits, int32_t *out_n, int64_t *out_total)
{
    return range_search(idx, RangeArgs{B, dim, q, min_cosine, max_hits, false, "orr_search_range_cosine"}, within, out_hits, out_n, out_total);
}

int orr_search_range_cosine_bulk(orr_index *idx, int32_t B, int32_t dim, const float *q, const double *min_cosine, const orr_scope *within,
                                 int32_t max_hits, orr_range_hit *out_hits, int32_t *out_n, int64_t *out_total)
{
    return range_search(idx, RangeArgs{B, dim, q, min_cosine, max_hits, true, "orr_search_range_cosine_bulk"}, within, out_hits, out_n, out_total);
}

// ---- diverse search (orr_search_batch_diverse, orr_index_pair_dots; the rules are orr_diverse_plan.h's) ----------------------
static_assert(diverse::kSelWidth == orr::kSelWidth, "diverse::kMaxPool is the ladder's largest take from one selection list");
static_assert(diverse::kMaxPool == ORR_DIVERSE_MAX_POOL && diverse::Collapse == ORR_DIVERSE_COLLAPSE && diverse::Mmr == ORR_DIVERSE_MMR, "the header's constants");

// The exact pair matrices of n_lists lists on the lane the caller holds: list l is cnt[l] <= stride positions pos[l * stride + i],
// every one of them checked against the shard's rows by the caller.  mats [n_lists][stride][stride]: the elements with i and j
// below cnt[l] are the kernel's, the others are whatever the workspace held.  Positions and lengths go up and the matrices come
// back through pinned memory, kListsPerLaunch lists a launch.  With `foreign` (the cluster's pair step): bit i of foreign[l] set
// says that pos[l * stride + i] is a row of the lane's ws_diverse_foreign, which holds n_foreign rows the other shards sent.
static int pair_dots_on_lane(orr_index *lane, int32_t n_lists, int32_t stride, const uint32_t *pos, const uint32_t *cnt, double *mats,
                             const uint64_t *foreign = nullptr, int64_t n_foreign = 0)
{
    constexpr int32_t kListsPerLaunch = 1024;
    if (n_lists <= 0) return ORR_OK;
    ORR_TRY(bind_device(lane));
    hipStream_t s = lane->stream;
    const int32_t D = lane->dim;
    const size_t per_pos = (size_t)stride, per_mat = (size_t)stride * (size_t)stride;
    const size_t group = (size_t)std::min<int32_t>(n_lists, kListsPerLaunch);
    const size_t pos_bytes = sizeof(uint32_t) * group * per_pos, cnt_bytes = sizeof(uint32_t) * group, mat_bytes = sizeof(double) * group * per_mat;
    const size_t msk_bytes = foreign ? sizeof(uint64_t) * group : 0, pin_msk_at = (pos_bytes + cnt_bytes + 7) / 8 * 8;
    const size_t pin_mat_at = (pin_msk_at + msk_bytes + 15) / 16 * 16;
    if (foreign) ORR_TRY(lane->ws_diverse_mask.reserve(msk_bytes));
    ORR_TRY(lane->ws_diverse_pos.reserve(pos_bytes));
    ORR_TRY(lane->ws_diverse_cnt.reserve(cnt_bytes));
    ORR_TRY(lane->ws_diverse_out.reserve(mat_bytes));
    ORR_TRY(lane->pin_diverse.reserve(pin_mat_at + mat_bytes));
    uint8_t *pin = lane->pin_diverse.as<uint8_t>();
    for (int32_t l0 = 0; l0 < n_lists; l0 += kListsPerLaunch) {
        const size_t nl = (size_t)std::min<int32_t>(kListsPerLaunch, n_lists - l0);
        double rows_read = 0.0, pairs = 0.0;
        for (size_t l = 0; l < nl; ++l) { rows_read += (double)cnt[(size_t)l0 + l]; pairs += (double)diverse::pair_count((int32_t)cnt[(size_t)l0 + l]); }
        memcpy(pin, pos + (size_t)l0 * per_pos, sizeof(uint32_t) * nl * per_pos);
        memcpy(pin + pos_bytes, cnt + l0, sizeof(uint32_t) * nl);
        HIP_TRY(hipMemcpyAsync(lane->ws_diverse_pos.p, pin, sizeof(uint32_t) * nl * per_pos, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(lane->ws_diverse_cnt.p, pin + pos_bytes, sizeof(uint32_t) * nl, hipMemcpyHostToDevice, s));
        if (foreign) {
            memcpy(pin + pin_msk_at, foreign + l0, sizeof(uint64_t) * nl);
            HIP_TRY(hipMemcpyAsync(lane->ws_diverse_mask.p, pin + pin_msk_at, sizeof(uint64_t) * nl, hipMemcpyHostToDevice, s));
        }
        {
            Timed t(lane, "pair_dots", 4.0 * rows_read * (double)D + 16.0 * pairs);
            if (foreign)
                HIP_TRY(orr::launch_pair_dots_two(lane->d_emb, lane->n_rows, lane->ws_diverse_foreign.as<float>(), n_foreign, D, lane->ws_diverse_pos.as<uint32_t>(),
                                                  lane->ws_diverse_cnt.as<uint32_t>(), lane->ws_diverse_mask.as<unsigned long long>(), (int32_t)nl, stride,
                                                  lane->ws_diverse_out.as<double>(), s));
            else
                HIP_TRY(orr::launch_pair_dots(lane->d_emb, lane->n_rows, D, lane->ws_diverse_pos.as<uint32_t>(), lane->ws_diverse_cnt.as<uint32_t>(),
                                              (int32_t)nl, stride, lane->ws_diverse_out.as<double>(), s));
        }
        HIP_TRY(hipMemcpyAsync(pin + pin_mat_at, lane->ws_diverse_out.p, sizeof(double) * nl * per_mat, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        collect_events(lane);
        memcpy(mats + (size_t)l0 * per_mat, pin + pin_mat_at, sizeof(double) * nl * per_mat);
    }
    return ORR_OK;
}

struct DiverseArgs {
    int32_t pool, mode;
    double param;
};

// orr_search_batch_diverse on the lane the caller holds (with the scope, if any, held shared):
//   1. the pool: the plain search (the masked search inside `within`) for topk = pool, unchanged, which also hands back every
//      result's order_key (BatchArgs::out_keys); position = order_key - row_base;
//   2. the queries whose greedy pass reads a cosine (diverse::needs_dots) send their pools to ONE launch_pair_dots per 1024 of
//      them; the matrices come back to the host;
//   3. the host forms c_ij = scope_near::cosine_of(dot_ij, dot_ii, dot_jj) -- the diagonal supplies both norms -- runs
//      diverse::select_collapse / select_mmr and writes the outputs.  A query that reads no cosine takes no launch.
static int diverse_run(orr_index *lane, const char *fn, const BatchArgs &a, const orr_scope *within, const DiverseArgs &d, int64_t *out_rows,
                       double *out_scores, int32_t *out_counts, int32_t *out_pool_rank)
{
    const int32_t B = a.B, pool = d.pool, take = diverse::take_of(a.topk);
    std::vector<int64_t> p_rows((size_t)B * pool, -1), p_keys((size_t)B * pool, -1);
    std::vector<double> p_scores((size_t)B * pool, 0.0);
    std::vector<int32_t> p_cnt((size_t)B, 0);
    BatchArgs pa = a;
    pa.topk = pool;
    pa.out_keys = p_keys.data();
    if (within) {
        ORR_TRY(masked_batch(lane, pa, ScopeSource{nullptr, within}, p_rows.data(), p_scores.data(), p_cnt.data()));
    } else {
        const int64_t n = participating_rows(lane, a.candidate_limit);
        ORR_TRY(escalate(index_backend(lane, fn, n), pa, escalation::initial_kprime(pool, n, orr::kSelWidth), p_rows.data(), p_scores.data(), p_cnt.data()));
    }
    // ---- the pools that are compared
    std::vector<int32_t> slot_of((size_t)B, -1);
    int32_t n_lists = 0, stride = 1;
    for (int32_t b = 0; b < B; ++b) {
        if (!diverse::needs_dots(d.mode, d.param, p_cnt[(size_t)b], lane->dim)) continue;
        slot_of[(size_t)b] = n_lists++;
        stride = std::max(stride, p_cnt[(size_t)b]);
    }
    std::vector<double> mats;
    if (n_lists > 0) {
        std::vector<uint32_t> pos((size_t)n_lists * stride, 0u), cnt((size_t)n_lists, 0u);
        for (int32_t b = 0; b < B; ++b) {
            const int32_t l = slot_of[(size_t)b];
            if (l < 0) continue;
            cnt[(size_t)l] = (uint32_t)p_cnt[(size_t)b];
            for (int32_t i = 0; i < p_cnt[(size_t)b]; ++i) {
                const int64_t p = p_keys[(size_t)b * pool + i] - lane->row_base;
                if (p < 0 || p >= lane->n_rows) return fail(ORR_EDEVICE, "%s: a result's order_key lies outside the shard", fn);
                pos[(size_t)l * stride + i] = (uint32_t)p;
            }
        }
        mats.resize((size_t)n_lists * stride * stride);
        ORR_TRY(pair_dots_on_lane(lane, n_lists, stride, pos.data(), cnt.data(), mats.data()));
    }
    // ---- the greedy pass and the outputs
    std::vector<int32_t> picks((size_t)take);
    for (int32_t b = 0; b < B; ++b) {
        const int32_t n = p_cnt[(size_t)b];
        const double *m = slot_of[(size_t)b] >= 0 ? mats.data() + (size_t)slot_of[(size_t)b] * stride * stride : nullptr;
        auto cosine = [m, stride](int32_t i, int32_t j) -> double {
            if (!m) return 0.0;
            return scope_near::cosine_of(m[diverse::mat_index(stride, i, j)], m[diverse::mat_index(stride, i, i)], m[diverse::mat_index(stride, j, j)]);
        };
        const int32_t kept = d.mode == diverse::Collapse ? diverse::select_collapse(n, take, d.param, cosine, picks.data())
                                                         : diverse::select_mmr(n, take, d.param, p_scores.data() + (size_t)b * pool, cosine, picks.data());
        for (int32_t i = 0; i < take; ++i) {
            const size_t o = (size_t)b * take + i;
            const bool have = i < kept;
            out_rows[o] = have ? p_rows[(size_t)b * pool + picks[(size_t)i]] : -1;
            out_scores[o] = have ? p_scores[(size_t)b * pool + picks[(size_t)i]] : 0.0;
            if (out_pool_rank) out_pool_rank[o] = have ? picks[(size_t)i] : -1;
        }
        out_counts[b] = kept;
    }
    return ORR_OK;
}

int orr_search_batch_diverse(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8, const uint32_t *term_off,
                             const uint32_t *query_term_off, int64_t now_ticks, int32_t topk, int64_t candidate_limit, const orr_scope *within,
                             int32_t pool, int32_t mode, double param, int64_t *out_rows, double *out_scores, int32_t *out_counts,
                             int32_t *out_pool_rank)
{
    static const char *fn = "orr_search_batch_diverse";
    switch (diverse::first_invalid(!out_rows || !out_scores || !out_counts, topk, pool, mode, param)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out_rows, out_scores and out_counts are required", fn);
    case 2: return fail(ORR_EINVAL, "%s: pool must be in 1 .. %d", fn, diverse::kMaxPool);
    case 3: return fail(ORR_EINVAL, "%s: topk %d exceeds the pool of %d", fn, topk, pool);
    case 4: return fail(ORR_EINVAL, "%s: mode must be ORR_DIVERSE_COLLAPSE (0) or ORR_DIVERSE_MMR (1)", fn);
    case 5: return fail(ORR_EINVAL, "%s: param is NaN", fn);
    default: return fail(ORR_EINVAL, "%s: lambda must be in [0, 1]", fn);
    }
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    if (B == 0) return ORR_OK;
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    ORR_TRY(check_batch(idx, a, fn));
    orr_index *own = nullptr;
    if (within) ORR_TRY(scope_owner(within, idx, fn, &own));
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    std::shared_lock<std::shared_mutex> rd;
    if (within) {
        rd = std::shared_lock<std::shared_mutex>(within->mu);
        ORR_TRY(scope_owner(within, idx, fn, &own));
        if (within->n_rows != idx->n_rows) return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)within->n_rows, (long long)idx->n_rows);
    }
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    const int r = diverse_run(idx, fn, a, within, DiverseArgs{pool, mode, param}, out_rows, out_scores, out_counts, out_pool_rank);
    g_ht.done();
    return r;
}

int orr_index_pair_dots(orr_index *idx, int32_t n_lists, const uint32_t *list_off, const int64_t *positions, int32_t stride, double *out)
{
    static const char *fn = "orr_index_pair_dots";
    switch (diverse::first_invalid_pairs(!out, n_lists, !list_off, !positions, stride)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out is NULL", fn);
    case 2: return fail(ORR_EINVAL, "%s: n_lists is negative", fn);
    case 3: return fail(ORR_EINVAL, "%s: stride must be in 1 .. %d", fn, diverse::kMaxPool);
    case 4: return fail(ORR_EINVAL, "%s: list_off is NULL", fn);
    default: return fail(ORR_EINVAL, "%s: positions is NULL", fn);
    }
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    if (list_off[0] != 0) return fail(ORR_EINVAL, "%s: list_off must start at 0", fn);
    for (int32_t l = 0; l < n_lists; ++l) {
        if (list_off[l + 1] < list_off[l]) return fail(ORR_EINVAL, "%s: list_off decreases at list %d", fn, l);
        if (list_off[l + 1] - list_off[l] > (uint32_t)stride) return fail(ORR_EINVAL, "%s: list %d holds %u positions, stride is %d", fn, l, list_off[l + 1] - list_off[l], stride);
    }
    Lane ln = acquire_lane(idx);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    if (!lane->sealed) return fail(ORR_ESTATE, "%s: the index is not sealed", fn);
    for (uint32_t e = 0; e < list_off[n_lists]; ++e)                          // before any launch: the kernel is never handed a row it cannot read
        if (positions[e] < 0 || positions[e] >= lane->n_rows)
            return fail(ORR_EINVAL, "%s: positions[%u] = %lld is outside 0 .. %lld", fn, e, (long long)positions[e], (long long)lane->n_rows - 1);
    if (n_lists == 0) return ORR_OK;
    std::vector<uint32_t> pos((size_t)n_lists * stride, 0u), cnt((size_t)n_lists, 0u);
    for (int32_t l = 0; l < n_lists; ++l) {
        cnt[(size_t)l] = list_off[l + 1] - list_off[l];
        for (uint32_t i = 0; i < cnt[(size_t)l]; ++i) pos[(size_t)l * stride + i] = (uint32_t)positions[list_off[l] + i];
    }
    std::vector<double> mats((size_t)n_lists * stride * stride, 0.0);
    if (lane->dim > 0) ORR_TRY(pair_dots_on_lane(lane, n_lists, stride, pos.data(), cnt.data(), mats.data()));
    for (int32_t l = 0; l < n_lists; ++l)                                     // (what lies at or beyond a list's length stays as the caller left it)
        for (uint32_t i = 0; i < cnt[(size_t)l]; ++i)
            memcpy(out + ((size_t)l * stride + i) * stride, mats.data() + ((size_t)l * stride + i) * stride, sizeof(double) * cnt[(size_t)l]);
    return ORR_OK;
}

// ---- row keys and the per-key search (orr_keys, orr_search_batch_per_key; the rules are orr_per_key_plan.h's) -----------------

static_assert(per_key::kSelWidth == orr::kSelWidth, "orr_per_key_plan.h restates the selection width");
static_assert(per_key::kMaxSlots <= orr::kMaxGatherGroups, "a slice's temporary scopes go through one grouped call");

// The shard of a key column, or the reason it cannot be used: ORR_ESTATE orphaned; with idx: ORR_EINVAL another shard.
static int keys_owner(const orr_keys *k, const orr_index *idx, const char *fn, orr_index **own)
{
    *own = k->owner.load();
    if (!*own) return fail(ORR_ESTATE, "%s: the keys are orphaned: their index was destroyed", fn);
    if (idx && owner_of(idx) != *own) return fail(ORR_EINVAL, "%s: the keys belong to another shard", fn);
    return ORR_OK;
}

// orr_keys_set behind its locks (the lane, its lock, the column exclusively): ids and keys (host or device, the same memory)
// come to the device, keys_scatter stores behind scope_lookup's search.
static int keys_set_held(orr_index *lane, orr_keys *k, int64_t n, const int64_t *row_ids, const int64_t *keys, int64_t *out_set)
{
    if (out_set) *out_set = 0;
    if (n <= 0 || lane->n_rows <= 0) return ORR_OK;
    ORR_TRY(bind_device(lane));
    ORR_TRY(ensure_scope_table(lane));
    const orr_index *own = owner_of(lane);
    hipStream_t s = lane->stream;
    DevBuf in;                                         // [ids x n][keys x n][counter]
    auto body = [&]() -> int {
        ORR_TRY(in.reserve(sizeof(int64_t) * (2 * (size_t)n + 1)));
        int64_t *d_ids = in.as<int64_t>(), *d_keys = d_ids + n;
        unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(d_keys + n);
        HIP_TRY(hipMemcpyAsync(d_ids, row_ids, sizeof(int64_t) * (size_t)n, hipMemcpyDefault, s));
        HIP_TRY(hipMemcpyAsync(d_keys, keys, sizeof(int64_t) * (size_t)n, hipMemcpyDefault, s));
        HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), s));
        {
            Timed t(lane, "keys_scatter", 24.0 * (double)n);
            HIP_TRY(orr::launch_keys_scatter(own->scope_tab_ids, own->scope_tab_pos, lane->n_rows, d_ids, d_keys, n, own->d_dead.as<int64_t>(),
                                             (int32_t)own->dead.size(), k->d_key, d_cnt, s));
        }
        unsigned long long cnt = 0;
        HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        collect_events(lane);
        if (out_set) *out_set = (int64_t)cnt;
        return ORR_OK;
    };
    const int r = body();
    if (r != ORR_OK) (void)hipStreamSynchronize(s);
    in.release();
    return r;
}

int orr_keys_create(orr_index *idx, int64_t n, const int64_t *row_ids, const int64_t *keys, orr_keys **out)
{
    static const char *fn = "orr_keys_create";
    if (!out) return fail(ORR_EINVAL, "%s: out is NULL", fn);
    if (n < 0) return fail(ORR_EINVAL, "%s: n is negative", fn);
    if (n > 0 && (!row_ids || !keys)) return fail(ORR_EINVAL, "%s: row_ids or keys is NULL with %lld entries", fn, (long long)n);
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    Lane ln = acquire_lane(idx);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    if (!lane->sealed) return fail(ORR_ESTATE, "%s: the index is not sealed", fn);
    ORR_TRY(bind_device(lane));
    orr_keys *k = new (std::nothrow) orr_keys();
    if (!k) return fail(ORR_ENOMEM, "out of host memory");
    k->n_rows = lane->n_rows;
    int r = dev_alloc(&k->d_key, (size_t)std::max<int64_t>(k->n_rows, 1));
    if (r == ORR_OK) {
        Timed t(lane, "keys_fill_none", 8.0 * (double)k->n_rows);
        if (orr::launch_keys_fill_none(k->d_key, k->n_rows, lane->stream) != hipSuccess) r = fail(ORR_EDEVICE, "%s: the fill failed", fn);
    }
    if (r == ORR_OK) r = keys_set_held(lane, k, n, row_ids, keys, nullptr);
    if (r == ORR_OK && hipStreamSynchronize(lane->stream) != hipSuccess) r = fail(ORR_EDEVICE, "%s: device failure", fn);
    if (r != ORR_OK) {
        (void)hipStreamSynchronize(lane->stream);
        (void)hipGetLastError();
        if (k->d_key) (void)hipFree(k->d_key);
        delete k;
        return r;
    }
    orr_index *own = const_cast<orr_index *>(owner_of(lane));
    k->owner.store(own);
    { std::lock_guard<std::mutex> g(own->scope_mu); own->key_cols.push_back(k); }
    *out = k;
    return ORR_OK;
}

int orr_keys_set(orr_keys *k, int64_t n, const int64_t *row_ids, const int64_t *keys, int64_t *out_set)
{
    static const char *fn = "orr_keys_set";
    if (n < 0) return fail(ORR_EINVAL, "%s: n is negative", fn);
    if (n > 0 && (!row_ids || !keys)) return fail(ORR_EINVAL, "%s: row_ids or keys is NULL with %lld entries", fn, (long long)n);
    if (!k) return fail(ORR_EINVAL, "%s: null keys", fn);
    orr_index *own = nullptr;
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::unique_lock<std::shared_mutex> w(k->mu);
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    return keys_set_held(lane, k, n, row_ids, keys, out_set);
}

// orr_keys_get behind its locks (the lane, its lock, the column shared): own is the column's shard.
static int keys_get_held(orr_index *lane, const orr_keys *k, const orr_index *own, int64_t n, const int64_t *row_ids, int64_t *out_keys)
{
    if (n == 0) return ORR_OK;
    if (lane->n_rows <= 0) { for (int64_t i = 0; i < n; ++i) out_keys[i] = ORR_KEY_NONE; return ORR_OK; }
    ORR_TRY(bind_device(lane));
    ORR_TRY(ensure_scope_table(lane));
    hipStream_t s = lane->stream;
    DevBuf io;                                         // [ids x n][keys x n]
    auto body = [&]() -> int {
        ORR_TRY(io.reserve(sizeof(int64_t) * 2 * (size_t)n));
        int64_t *d_ids = io.as<int64_t>(), *d_out = d_ids + n;
        HIP_TRY(hipMemcpyAsync(d_ids, row_ids, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, s));
        {
            Timed t(lane, "keys_gather", 24.0 * (double)n);
            HIP_TRY(orr::launch_keys_gather(k->d_key, lane->n_rows, d_ids, n, own->scope_tab_ids, own->scope_tab_pos, own->d_dead.as<int64_t>(),
                                            (int32_t)own->dead.size(), d_out, s));
        }
        HIP_TRY(hipMemcpyAsync(out_keys, d_out, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        collect_events(lane);
        return ORR_OK;
    };
    const int r = body();
    if (r != ORR_OK) (void)hipStreamSynchronize(s);
    io.release();
    return r;
}

int orr_keys_get(orr_keys *k, int64_t n, const int64_t *row_ids, int64_t *out_keys)
{
    static const char *fn = "orr_keys_get";
    if (n < 0) return fail(ORR_EINVAL, "%s: n is negative", fn);
    if (n > 0 && (!row_ids || !out_keys)) return fail(ORR_EINVAL, "%s: row_ids or out_keys is NULL with %lld entries", fn, (long long)n);
    if (!k) return fail(ORR_EINVAL, "%s: null keys", fn);
    orr_index *own = nullptr;
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rd(k->mu);
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    return keys_get_held(lane, k, own, n, row_ids, out_keys);
}

int64_t orr_keys_rows(const orr_keys *k)
{
    if (!k) return -1;
    orr_index *own = k->owner.load();
    if (!own) return -1;
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rd(k->mu);
    if (!k->owner.load()) return -1;
    if (lane->n_rows <= 0) return 0;
    if (bind_device(lane) != ORR_OK) return -1;
    hipStream_t s = lane->stream;
    DevBuf cnt;
    unsigned long long h = 0;
    bool ok = cnt.reserve(sizeof(unsigned long long)) == ORR_OK && hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), s) == hipSuccess;
    if (ok) {
        Timed t(lane, "keys_count", 8.0 * (double)lane->n_rows);
        ok = orr::launch_keys_count(k->d_key, lane->n_rows, own->d_dead.as<int64_t>(), (int32_t)own->dead.size(), cnt.as<unsigned long long>(), s) == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(&h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    collect_events(lane);
    cnt.release();
    return ok ? (int64_t)h : -1;
}

void orr_keys_destroy(orr_keys *k)
{
    if (!k) return;
    std::lock_guard<std::mutex> life(g_scope_life_mu); // (the owning index is not destroyed meanwhile)
    orr_index *own = k->owner.load();
    if (own) {                                         // (the shard's maintenance holds scope_mu while it walks its columns)
        std::lock_guard<std::mutex> g(own->scope_mu);
        own->key_cols.erase(std::remove(own->key_cols.begin(), own->key_cols.end(), k), own->key_cols.end());
    }
    {
        std::unique_lock<std::shared_mutex> w(k->mu);  // waits for the searches that hold it
        if (k->owner.load()) {
            (void)hipSetDevice(own->device);
            if (k->d_key) (void)hipFree(k->d_key);
        }
        k->d_key = nullptr;
    }
    delete k;
}

int orr_scope_create_keys(orr_index *idx, const orr_keys *k, int32_t n_keys, const int64_t *keys, orr_scope **out)
{
    static const char *fn = "orr_scope_create_keys";
    switch (per_key::first_invalid_scope_keys(!out, n_keys, !keys, !k)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out is NULL", fn);
    case 2: return fail(ORR_EINVAL, "%s: n_keys must be in 0 .. %d", fn, per_key::kMaxScopeKeys);
    case 3: return fail(ORR_EINVAL, "%s: keys is NULL with %d keys", fn, n_keys);
    default: return fail(ORR_EINVAL, "%s: null keys handle", fn);
    }
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    orr_index *own = nullptr;
    ORR_TRY(keys_owner(k, idx, fn, &own));
    const std::vector<int64_t> table = per_key::member_table(keys, n_keys);
    return make_scope(idx, fn, out, [&](orr_index *lane, orr_scope *sc) -> int {
        std::shared_lock<std::shared_mutex> rd(k->mu);
        ORR_TRY(keys_owner(k, lane, fn, &own));
        if (k->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the keys cover %lld rows, the handle %lld", fn, (long long)k->n_rows, (long long)lane->n_rows);
        const orr_index *o = owner_of(lane);
        hipStream_t s = lane->stream;
        if (table.empty() || lane->n_rows <= 0) {      // the empty scope
            HIP_TRY(hipMemsetAsync(sc->bm, 0, sizeof(uint32_t) * (size_t)sc->words, s));
            return ORR_OK;
        }
        DevBuf tab;
        auto body = [&]() -> int {
            ORR_TRY(tab.reserve(sizeof(int64_t) * table.size()));
            HIP_TRY(hipMemcpyAsync(tab.p, table.data(), sizeof(int64_t) * table.size(), hipMemcpyHostToDevice, s));
            {
                Timed t(lane, "keys_member", 8.0 * (double)lane->n_rows + 4.0 * (double)sc->words);
                HIP_TRY(orr::launch_keys_member(k->d_key, lane->n_rows, tab.as<int64_t>(), (int32_t)table.size(), sc->bm, sc->words, s));
            }
            {
                Timed t(lane, "scope_clear_positions", 12.0 * (double)o->dead.size());
                HIP_TRY(orr::launch_scope_clear_positions(sc->bm, sc->words, o->d_dead.as<int64_t>(), (int64_t)o->dead.size(), s));
            }
            HIP_TRY(hipStreamSynchronize(s));          // (the table goes with this frame)
            return ORR_OK;
        };
        const int r = body();
        if (r != ORR_OK) (void)hipStreamSynchronize(s);
        tab.release();
        return r;
    });
}

// ---- key groups (orr_keys_groups, orr_keys_centroids, orr_scope_centroid; the rules are orr_key_groups_plan.h's) ---------------

static_assert(key_groups::kMaxKeys == per_key::kMaxScopeKeys, "orr_keys_centroids lists as many keys as orr_scope_create_keys");
static_assert(key_groups::kBlock == ORR_KEY_GROUPS_BLOCK, "the header states the block of the sum");

namespace {

// What one key-groups call owns on the device; everything goes with the call.
struct KeyGroupsWork {
    DevBuf live_bm, tab, counts, offsets, key_a, key_b, pos_a, pos_b, tmp, run_key, run_len, run_n, blocks, folds, sums, parts;
    const uint32_t *pos = nullptr;                     // the pairs' positions in their final order
    const uint64_t *key = nullptr;                     // ... and their keys (modes 0 and 1)
    ~KeyGroupsWork()
    {
        for (DevBuf *b : {&live_bm, &tab, &counts, &offsets, &key_a, &key_b, &pos_a, &pos_b, &tmp, &run_key, &run_len, &run_n, &blocks, &folds, &sums, &parts})
            b->release();
    }
};

// The call's selected rows as pairs in candidate order (launch_keys_pairs: mode 0 the rows with a key, 1 the participating rows
// whose key is in `table`, 2 the participating rows of `within`, 3 the participating rows with a key), sorted by key for modes
// 0, 1 and 3 (stable: positions stay ascending within a key).  *out_m = their number; ends synchronised.
int key_groups_pairs(orr_index *lane, const orr_keys *k, const orr_scope *within, int32_t mode, const std::vector<int64_t> *table,
                     KeyGroupsWork &w, int64_t *out_m)
{
    *out_m = 0;
    const orr_index *own = owner_of(lane);
    hipStream_t s = lane->stream;
    const int64_t n = lane->n_rows;
    if (n <= 0) return ORR_OK;
    if (n > (int64_t)0x7FFFFFFF) return fail(ORR_ELIMIT, "key groups: a shard of %lld rows is beyond 2^31 - 1", (long long)n);
    const uint32_t *bm = nullptr;
    int64_t words = 0;
    if (within) {
        bm = within->bm; words = within->words;
    } else {                                           // the live rows
        words = (int64_t)(scope::bitmap_bytes(n) / 4);
        ORR_TRY(w.live_bm.reserve(sizeof(uint32_t) * (size_t)words));
        {
            Timed t(lane, "scope_fill_range", 4.0 * (double)words);
            HIP_TRY(orr::launch_scope_fill_range(w.live_bm.as<uint32_t>(), words, 0, n, s));
        }
        {
            Timed t(lane, "scope_clear_positions", 12.0 * (double)own->dead.size());
            HIP_TRY(orr::launch_scope_clear_positions(w.live_bm.as<uint32_t>(), words, own->d_dead.as<int64_t>(), (int64_t)own->dead.size(), s));
        }
        bm = w.live_bm.as<uint32_t>();
    }
    const int32_t n_tab = table ? (int32_t)table->size() : 0;
    if (mode == 1) {
        ORR_TRY(w.tab.reserve(sizeof(int64_t) * (size_t)n_tab));
        HIP_TRY(hipMemcpyAsync(w.tab.p, table->data(), sizeof(int64_t) * (size_t)n_tab, hipMemcpyHostToDevice, s));
    }
    const int64_t *d_key = k ? k->d_key : nullptr;
    const int64_t nb = orr::key_groups_pair_blocks(n);
    ORR_TRY(w.counts.reserve(sizeof(uint32_t) * (size_t)(nb + 1)));
    ORR_TRY(w.offsets.reserve(sizeof(uint32_t) * (size_t)(nb + 1)));
    HIP_TRY(hipMemsetAsync(w.counts.as<uint32_t>() + nb, 0, sizeof(uint32_t), s));      // the closing entry: its offset is the total
    const double pass_bytes = (mode == 2 ? 8.0 : 16.0) * (double)n + 4.0 * (double)words;
    {
        Timed t(lane, "keys_pairs_count", pass_bytes);
        HIP_TRY(orr::launch_keys_pairs(mode, false, d_key, lane->d_norm_b, n, bm, words, w.tab.as<int64_t>(), n_tab, w.counts.as<uint32_t>(), nullptr, 0,
                                       nullptr, nullptr, s));
    }
    size_t tmp_bytes = 0;
    HIP_TRY(orr::keys_pairs_scan(nullptr, tmp_bytes, w.counts.as<uint32_t>(), w.offsets.as<uint32_t>(), nb + 1, s));
    ORR_TRY(w.tmp.reserve(std::max<size_t>(tmp_bytes, 16)));
    {
        Timed t(lane, "keys_pairs_scan", 8.0 * (double)(nb + 1));
        HIP_TRY(orr::keys_pairs_scan(w.tmp.p, tmp_bytes, w.counts.as<uint32_t>(), w.offsets.as<uint32_t>(), nb + 1, s));
    }
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, w.offsets.as<uint32_t>() + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int64_t m = (int64_t)total;
    if (m > n) return fail(ORR_EDEVICE, "key groups: %lld pairs of %lld rows", (long long)m, (long long)n);
    *out_m = m;
    if (m == 0) return ORR_OK;
    ORR_TRY(w.pos_a.reserve(sizeof(uint32_t) * (size_t)m));
    if (mode != 2) ORR_TRY(w.key_a.reserve(sizeof(uint64_t) * (size_t)m));
    {
        Timed t(lane, "keys_pairs", pass_bytes + (mode == 2 ? 4.0 : 12.0) * (double)m);
        HIP_TRY(orr::launch_keys_pairs(mode, true, d_key, lane->d_norm_b, n, bm, words, w.tab.as<int64_t>(), n_tab, nullptr, w.offsets.as<uint32_t>(), m,
                                       w.key_a.as<uint64_t>(), w.pos_a.as<uint32_t>(), s));
    }
    w.pos = w.pos_a.as<uint32_t>();
    w.key = w.key_a.as<uint64_t>();
    if (mode == 2) return ORR_OK;
    ORR_TRY(w.pos_b.reserve(sizeof(uint32_t) * (size_t)m));
    ORR_TRY(w.key_b.reserve(sizeof(uint64_t) * (size_t)m));
    const int32_t end_bit = mode == 1 ? key_groups::table_bits(n_tab) : 64;
    tmp_bytes = 0;
    HIP_TRY(orr::keys_pairs_sort(nullptr, tmp_bytes, w.key_a.as<uint64_t>(), w.key_b.as<uint64_t>(), w.pos_a.as<uint32_t>(), w.pos_b.as<uint32_t>(), m, end_bit, s));
    ORR_TRY(w.tmp.reserve(std::max<size_t>(tmp_bytes, 16)));
    {
        Timed t(lane, "keys_pairs_sort", 24.0 * (double)m * (double)((end_bit + 7) / 8));
        HIP_TRY(orr::keys_pairs_sort(w.tmp.p, tmp_bytes, w.key_a.as<uint64_t>(), w.key_b.as<uint64_t>(), w.pos_a.as<uint32_t>(), w.pos_b.as<uint32_t>(), m, end_bit, s));
    }
    w.pos = w.pos_b.as<uint32_t>();
    w.key = w.key_b.as<uint64_t>();
    return ORR_OK;
}

// The runs of the sorted pairs' keys: run_key / run_len on the device, *out_runs their number; ends synchronised.
int key_groups_runs(orr_index *lane, KeyGroupsWork &w, int64_t m, int64_t *out_runs)
{
    hipStream_t s = lane->stream;
    *out_runs = 0;
    if (m <= 0) return ORR_OK;
    ORR_TRY(w.run_key.reserve(sizeof(uint64_t) * (size_t)m));
    ORR_TRY(w.run_len.reserve(sizeof(uint32_t) * (size_t)m));
    ORR_TRY(w.run_n.reserve(sizeof(uint32_t)));
    size_t tmp_bytes = 0;
    HIP_TRY(orr::keys_pairs_runs(nullptr, tmp_bytes, w.key, w.run_key.as<uint64_t>(), w.run_len.as<uint32_t>(), w.run_n.as<uint32_t>(), m, s));
    ORR_TRY(w.tmp.reserve(std::max<size_t>(tmp_bytes, 16)));
    {
        Timed t(lane, "keys_runs", 8.0 * (double)m);
        HIP_TRY(orr::keys_pairs_runs(w.tmp.p, tmp_bytes, w.key, w.run_key.as<uint64_t>(), w.run_len.as<uint32_t>(), w.run_n.as<uint32_t>(), m, s));
    }
    uint32_t runs = 0;
    HIP_TRY(hipMemcpyAsync(&runs, w.run_n.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((int64_t)runs > m) return fail(ORR_EDEVICE, "key groups: %u runs of %lld pairs", runs, (long long)m);
    *out_runs = (int64_t)runs;
    return ORR_OK;
}

// The launch half of one slice's sums: the blocks (at least one) and folds brought to the device, keys_block_sums,
// keys_block_fold where a key has several blocks; the n_slots x dim sums stay on the device (a key without a block reads +0.0).
// Nothing is waited for: the host's blocks and folds live until the caller has synchronised.
int key_groups_slice_launch(orr_index *lane, KeyGroupsWork &w, int32_t n_slots, const std::vector<key_groups::Block> &blocks,
                            const std::vector<key_groups::Fold> &folds, uint32_t n_parts)
{
    hipStream_t s = lane->stream;
    const int32_t dim = lane->dim;
    const size_t sum_bytes = sizeof(double) * (size_t)std::max(n_slots, 1) * (size_t)dim;
    ORR_TRY(w.sums.reserve(sum_bytes));
    ORR_TRY(w.blocks.reserve(sizeof(key_groups::Block) * blocks.size()));
    if (n_parts) ORR_TRY(w.parts.reserve(sizeof(double) * (size_t)n_parts * (size_t)dim));
    if (!folds.empty()) ORR_TRY(w.folds.reserve(sizeof(key_groups::Fold) * folds.size()));
    HIP_TRY(hipMemsetAsync(w.sums.p, 0, sum_bytes, s));
    HIP_TRY(hipMemcpyAsync(w.blocks.p, blocks.data(), sizeof(key_groups::Block) * blocks.size(), hipMemcpyHostToDevice, s));
    if (!folds.empty()) HIP_TRY(hipMemcpyAsync(w.folds.p, folds.data(), sizeof(key_groups::Fold) * folds.size(), hipMemcpyHostToDevice, s));
    double rows = 0.0;
    for (const key_groups::Block &b : blocks) rows += (double)b.len;
    {
        Timed t(lane, "keys_block_sums", 4.0 * rows * (double)dim + 8.0 * (double)blocks.size() * (double)dim);
        HIP_TRY(orr::launch_keys_block_sums(lane->d_emb, lane->n_rows, dim, w.pos, w.blocks.as<key_groups::Block>(), (int64_t)blocks.size(),
                                            w.sums.as<double>(), w.parts.as<double>(), s));
    }
    if (!folds.empty()) {
        Timed t(lane, "keys_block_fold", 8.0 * ((double)n_parts + (double)folds.size()) * (double)dim);
        HIP_TRY(orr::launch_keys_block_fold(w.folds.as<key_groups::Fold>(), (int64_t)folds.size(), w.parts.as<double>(), dim, w.sums.as<double>(), s));
    }
    return ORR_OK;
}

// One slice's sums: key_groups_slice_launch, then the n_slots x dim sums back in `host`.  Ends synchronised.
int key_groups_slice_sums(orr_index *lane, KeyGroupsWork &w, int32_t n_slots, const std::vector<key_groups::Block> &blocks,
                          const std::vector<key_groups::Fold> &folds, uint32_t n_parts, double *host)
{
    hipStream_t s = lane->stream;
    const size_t sum_bytes = sizeof(double) * (size_t)n_slots * (size_t)lane->dim;
    if (blocks.empty()) { memset(host, 0, sum_bytes); return ORR_OK; }
    ORR_TRY(key_groups_slice_launch(lane, w, n_slots, blocks, folds, n_parts));
    HIP_TRY(hipMemcpyAsync(host, w.sums.p, sum_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                  // (the host's blocks and folds go with this frame)
    return ORR_OK;
}

// `within` beside the keys of shard `own`, behind the lane's lock and both handles' shared locks
int key_groups_check_scope(const orr_scope *within, const orr_index *lane, const char *fn)
{
    if (!within) return ORR_OK;
    orr_index *sown = nullptr;
    ORR_TRY(scope_owner(within, lane, fn, &sown));
    if (within->n_rows != lane->n_rows)
        return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)within->n_rows, (long long)lane->n_rows);
    return ORR_OK;
}

}  // namespace

int orr_keys_groups(orr_keys *k, const orr_scope *within, int64_t cap, int64_t *out_keys, int64_t *out_rows, int64_t *out_n, int64_t *out_total)
{
    static const char *fn = "orr_keys_groups";
    switch (key_groups::first_invalid_groups(cap, !out_keys, !out_rows, !out_n, !out_total, !k)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: cap is negative", fn);
    case 2: return fail(ORR_EINVAL, "%s: out_n or out_total is NULL", fn);
    case 3: return fail(ORR_EINVAL, "%s: out_keys or out_rows is NULL with room for %lld keys", fn, (long long)cap);
    default: return fail(ORR_EINVAL, "%s: null keys", fn);
    }
    orr_index *own = nullptr;
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rs;                            // the scope first, then the keys, as orr_search_batch_per_key
    if (within) rs = std::shared_lock<std::shared_mutex>(within->mu);
    std::shared_lock<std::shared_mutex> rd(k->mu);
    if (within) ORR_TRY(key_groups_check_scope(within, own, fn));      // (another shard: ORR_EINVAL; orphaned: ORR_ESTATE)
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    if (k->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the keys cover %lld rows, the handle %lld", fn, (long long)k->n_rows, (long long)lane->n_rows);
    ORR_TRY(bind_device(lane));
    hipStream_t s = lane->stream;
    KeyGroupsWork w;
    int64_t runs = 0;
    auto body = [&]() -> int {
        int64_t m = 0;
        ORR_TRY(key_groups_pairs(lane, k, within, 0, nullptr, w, &m));
        ORR_TRY(key_groups_runs(lane, w, m, &runs));
        const int64_t take = std::min(runs, cap);
        if (take > 0) {
            std::vector<uint32_t> len((size_t)take);
            HIP_TRY(hipMemcpyAsync(out_keys, w.run_key.p, sizeof(uint64_t) * (size_t)take, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(len.data(), w.run_len.p, sizeof(uint32_t) * (size_t)take, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (int64_t i = 0; i < take; ++i) {
                out_keys[i] = key_groups::key_of_sort((uint64_t)out_keys[i]);
                out_rows[i] = (int64_t)len[(size_t)i];
            }
        }
        return ORR_OK;
    };
    const int r = body();
    (void)hipStreamSynchronize(s);
    collect_events(lane);
    if (r != ORR_OK) return r;
    *out_total = runs;
    *out_n = std::min(runs, cap);
    return ORR_OK;
}

int orr_keys_centroids(orr_keys *k, const orr_scope *within, int32_t n_keys, const int64_t *keys, int32_t dim, float *out_centroids,
                       double *out_sums, int64_t *out_used)
{
    static const char *fn = "orr_keys_centroids";
    switch (key_groups::first_invalid_centroids(n_keys, !keys, !out_used, !k)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: n_keys must be in 0 .. %d", fn, key_groups::kMaxKeys);
    case 2: return fail(ORR_EINVAL, "%s: keys is NULL with %d keys", fn, n_keys);
    case 3: return fail(ORR_EINVAL, "%s: out_used is NULL with %d keys", fn, n_keys);
    default: return fail(ORR_EINVAL, "%s: null keys", fn);
    }
    orr_index *own = nullptr;
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rs;                            // the scope first, then the keys, as orr_search_batch_per_key
    if (within) rs = std::shared_lock<std::shared_mutex>(within->mu);
    std::shared_lock<std::shared_mutex> rd(k->mu);
    if (within) ORR_TRY(key_groups_check_scope(within, own, fn));
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    if (k->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the keys cover %lld rows, the handle %lld", fn, (long long)k->n_rows, (long long)lane->n_rows);
    if (dim <= 0 || dim != lane->dim) return fail(ORR_EDIM, "%s: dim %d differs from the index dimension %d (and must be greater than 0)", fn, dim, lane->dim);
    if (n_keys == 0) return ORR_OK;
    ORR_TRY(bind_device(lane));
    hipStream_t s = lane->stream;
    // the sorted table of the distinct keys listed; the listed keys in the table's order (a key listed twice is answered twice)
    const std::vector<int64_t> table = per_key::member_table(keys, n_keys);
    const int32_t T = (int32_t)table.size();
    std::vector<int32_t> slot_of((size_t)n_keys), by_slot((size_t)n_keys);
    for (int32_t i = 0; i < n_keys; ++i) { slot_of[(size_t)i] = per_key::table_find(table.data(), T, keys[i]); by_slot[(size_t)i] = i; }
    std::stable_sort(by_slot.begin(), by_slot.end(), [&](int32_t a, int32_t b) { return slot_of[(size_t)a] < slot_of[(size_t)b]; });
    KeyGroupsWork w;
    std::vector<int64_t> first((size_t)T, 0), count((size_t)T, 0);
    std::vector<double> sums;
    std::vector<float> cent((size_t)dim);
    auto body = [&]() -> int {
        int64_t m = 0, runs = 0;
        ORR_TRY(key_groups_pairs(lane, k, within, 1, &table, w, &m));
        ORR_TRY(key_groups_runs(lane, w, m, &runs));
        if (runs > T) return fail(ORR_EDEVICE, "%s: %lld runs of %d keys", fn, (long long)runs, T);
        if (runs > 0) {
            std::vector<uint64_t> rk((size_t)runs);
            std::vector<uint32_t> rl((size_t)runs);
            HIP_TRY(hipMemcpyAsync(rk.data(), w.run_key.p, sizeof(uint64_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(rl.data(), w.run_len.p, sizeof(uint32_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            int64_t at = 0;
            for (int64_t i = 0; i < runs; ++i) {
                if (rk[(size_t)i] >= (uint64_t)T || at + (int64_t)rl[(size_t)i] > m) return fail(ORR_EDEVICE, "%s: a run outside the table", fn);
                first[(size_t)rk[(size_t)i]] = at;
                count[(size_t)rk[(size_t)i]] = (int64_t)rl[(size_t)i];
                at += (int64_t)rl[(size_t)i];
            }
        }
        const int32_t per_slice = key_groups::slice_keys(dim, lane->opt_key_groups_slice);
        sums.resize((size_t)std::min(per_slice, T) * (size_t)dim);
        std::vector<key_groups::Block> blocks;
        std::vector<key_groups::Fold> folds;
        size_t next = 0;                               // of by_slot
        for (int32_t s0 = 0; s0 < T; s0 += per_slice) {
            const int32_t ns = std::min(per_slice, T - s0);
            blocks.clear(); folds.clear();
            uint32_t n_parts = 0;
            for (int32_t j = 0; j < ns; ++j) key_groups::blocks_of(count[(size_t)(s0 + j)], first[(size_t)(s0 + j)], (uint32_t)j, blocks, folds, n_parts);
            ORR_TRY(key_groups_slice_sums(lane, w, ns, blocks, folds, n_parts, sums.data()));
            for (; next < by_slot.size() && slot_of[(size_t)by_slot[next]] < s0 + ns; ++next) {
                const int32_t i = by_slot[next], j = slot_of[(size_t)i] - s0;
                const double *S = sums.data() + (size_t)j * (size_t)dim;
                const int64_t used = count[(size_t)(s0 + j)];
                out_used[i] = used;
                if (out_sums) memcpy(out_sums + (size_t)i * (size_t)dim, S, sizeof(double) * (size_t)dim);
                if (out_centroids) key_groups::finish(S, used, dim, out_centroids + (size_t)i * (size_t)dim);
            }
        }
        return ORR_OK;
    };
    const int r = body();
    (void)hipStreamSynchronize(s);
    collect_events(lane);
    return r;
}

int orr_scope_centroid(orr_scope *sc, int32_t dim, float *out_centroid, double *out_sum, int64_t *out_used)
{
    static const char *fn = "orr_scope_centroid";
    switch (key_groups::first_invalid_scope_centroid(!out_used, !sc)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out_used is NULL", fn);
    default: return fail(ORR_EINVAL, "%s: null scope", fn);
    }
    orr_index *own = nullptr;
    ORR_TRY(scope_owner(sc, nullptr, fn, &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rd(sc->mu);
    ORR_TRY(scope_owner(sc, nullptr, fn, &own));
    if (sc->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)sc->n_rows, (long long)lane->n_rows);
    if (dim <= 0 || dim != lane->dim) return fail(ORR_EDIM, "%s: dim %d differs from the index dimension %d (and must be greater than 0)", fn, dim, lane->dim);
    ORR_TRY(bind_device(lane));
    hipStream_t s = lane->stream;
    KeyGroupsWork w;
    std::vector<double> sum((size_t)dim, 0.0);
    int64_t m = 0;
    auto body = [&]() -> int {
        ORR_TRY(key_groups_pairs(lane, nullptr, sc, 2, nullptr, w, &m));
        std::vector<key_groups::Block> blocks;
        std::vector<key_groups::Fold> folds;
        uint32_t n_parts = 0;
        key_groups::blocks_of(m, 0, 0u, blocks, folds, n_parts);
        return key_groups_slice_sums(lane, w, 1, blocks, folds, n_parts, sum.data());
    };
    const int r = body();
    (void)hipStreamSynchronize(s);
    collect_events(lane);
    if (r != ORR_OK) return r;
    *out_used = m;
    if (out_sum) memcpy(out_sum, sum.data(), sizeof(double) * (size_t)dim);
    if (out_centroid) key_groups::finish(sum.data(), m, dim, out_centroid);
    return ORR_OK;
}

// ---- the document index (orr_keys_centroid_index, orr_index_get_rows; the rules are orr_centroid_index_plan.h's) ----------------

namespace {

// What orr_keys_centroid_index owns on the device besides its key-groups work: a slice's kept keys, their fp32 centroids and ticks.
struct CentroidIndexWork {
    DevBuf kept, cent, ticks;
    ~CentroidIndexWork()
    {
        for (DevBuf *b : {&kept, &cent, &ticks}) b->release();
    }
};

// The body of orr_keys_centroid_index behind its locks: `res` is the fresh index the slices are appended to.  No sum and no
// centroid leaves the device: the host sees the keys, the run lengths and (inside orr_index_append) the ticks.
int centroid_index_fill(orr_index *lane, const orr_keys *k, const orr_scope *within, orr_index *res, int64_t *docs, int64_t *skipped)
{
    static const char *fn = "orr_keys_centroid_index";
    hipStream_t s = lane->stream;
    const int32_t dim = lane->dim;
    // everything a queued copy or launch may still touch lives until the stream is synchronised below, on every path
    KeyGroupsWork wa, w;
    CentroidIndexWork cw;
    std::vector<uint64_t> all, rk, no_content;
    std::vector<uint32_t> rl;
    std::vector<int64_t> used, first, ids;
    std::vector<key_groups::Block> blocks;
    std::vector<key_groups::Fold> folds;
    std::vector<centroid_index::Kept> kept;
    auto body = [&]() -> int {
        // all distinct keys of the members, ascending (orr_keys_groups' list) ...
        int64_t m0 = 0, T = 0;
        ORR_TRY(key_groups_pairs(lane, k, within, 0, nullptr, wa, &m0));
        ORR_TRY(key_groups_runs(lane, wa, m0, &T));
        all.resize((size_t)T);
        if (T > 0) {
            HIP_TRY(hipMemcpyAsync(all.data(), wa.run_key.p, sizeof(uint64_t) * (size_t)T, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        // ... and the participating members sorted by the same key: each key's count and the pair its run starts at
        int64_t m = 0, runs = 0;
        ORR_TRY(key_groups_pairs(lane, k, within, 3, nullptr, w, &m));
        ORR_TRY(key_groups_runs(lane, w, m, &runs));
        rk.resize((size_t)runs);
        rl.resize((size_t)runs);
        if (runs > 0) {
            HIP_TRY(hipMemcpyAsync(rk.data(), w.run_key.p, sizeof(uint64_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(rl.data(), w.run_len.p, sizeof(uint32_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (!centroid_index::merge_runs(all.data(), T, rk.data(), rl.data(), runs, m, used, first))
            return fail(ORR_EDEVICE, "%s: the participating runs do not fit the keys", fn);
        const int32_t per_slice = key_groups::slice_keys(dim, lane->opt_key_groups_slice);
        for (const centroid_index::Slice &sl : centroid_index::walk(used.data(), T, per_slice)) {
            if (sl.n_kept == 0) continue;              // (every key of the slice is skipped: nothing to launch, nothing to append)
            blocks.clear(); folds.clear(); kept.clear(); ids.clear();
            uint32_t n_parts = 0;
            for (int32_t j = 0; j < sl.n_keys; ++j)
                key_groups::blocks_of(used[(size_t)(sl.key0 + j)], first[(size_t)(sl.key0 + j)], (uint32_t)j, blocks, folds, n_parts);
            centroid_index::slice_kept(used.data(), first.data(), sl.key0, sl.n_keys, kept);
            for (const centroid_index::Kept &kk : kept) ids.push_back(key_groups::key_of_sort(all[(size_t)sl.key0 + kk.slot]));
            const size_t nk = kept.size();
            ORR_TRY(key_groups_slice_launch(lane, w, sl.n_keys, blocks, folds, n_parts));
            ORR_TRY(cw.kept.reserve(sizeof(centroid_index::Kept) * nk));
            ORR_TRY(cw.cent.reserve(sizeof(float) * nk * (size_t)dim));
            ORR_TRY(cw.ticks.reserve(sizeof(int64_t) * nk));
            HIP_TRY(hipMemcpyAsync(cw.kept.p, kept.data(), sizeof(centroid_index::Kept) * nk, hipMemcpyHostToDevice, s));
            {
                Timed t(lane, "keys_centroid_finish", (8.0 + 4.0) * (double)dim * (double)nk);
                HIP_TRY(orr::launch_keys_centroid_finish(w.sums.as<double>(), dim, cw.kept.as<centroid_index::Kept>(), (int64_t)nk, w.pos, lane->d_created,
                                                         cw.cent.as<float>(), cw.ticks.as<int64_t>(), s));
            }
            HIP_TRY(hipStreamSynchronize(s));          // (the append runs on the result's stream; the next slice reuses the host's tables)
            no_content.assign(nk + 1, 0);
            ORR_TRY(orr_index_append(res, (int64_t)nk, dim, cw.cent.as<float>(), cw.ticks.as<int64_t>(), nullptr, no_content.data(), ids.data()));
            *docs += (int64_t)nk;
        }
        *skipped = T - *docs;
        return ORR_OK;
    };
    const int r = body();
    (void)hipStreamSynchronize(s);                     // (an early return may have left copies and launches queued)
    return r;
}

}  // namespace

int orr_keys_centroid_index(orr_keys *k, const orr_scope *within, orr_index **out, int64_t *out_docs, int64_t *out_skipped)
{
    static const char *fn = "orr_keys_centroid_index";
    switch (centroid_index::first_invalid(!out, !k)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out is NULL", fn);
    default: return fail(ORR_EINVAL, "%s: null keys", fn);
    }
    orr_index *own = nullptr;
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    Lane ln = acquire_lane(own);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    std::shared_lock<std::shared_mutex> rs;                            // the scope first, then the keys, as orr_keys_centroids
    if (within) rs = std::shared_lock<std::shared_mutex>(within->mu);
    std::shared_lock<std::shared_mutex> rd(k->mu);
    if (within) ORR_TRY(key_groups_check_scope(within, own, fn));
    ORR_TRY(keys_owner(k, nullptr, fn, &own));
    if (k->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the keys cover %lld rows, the handle %lld", fn, (long long)k->n_rows, (long long)lane->n_rows);
    if (lane->dim <= 0) return fail(ORR_EDIM, "%s: the index has no embeddings (dim 0)", fn);
    ORR_TRY(bind_device(lane));
    orr_config cfg{};
    cfg.struct_size = (int32_t)sizeof(orr_config);
    cfg.device = own->device;
    cfg.dim = own->dim;
    orr_index *res = nullptr;
    ORR_TRY(orr_index_create(&cfg, &res));
    int64_t docs = 0, skipped = 0;
    int r = centroid_index_fill(lane, k, within, res, &docs, &skipped);
    (void)hipStreamSynchronize(lane->stream);
    collect_events(lane);
    if (r == ORR_OK) r = orr_index_seal(res);
    if (r != ORR_OK) {                                 // (the partial index goes; *out is not written)
        orr_index_destroy(res);
        return r;
    }
    *out = res;
    if (out_docs) *out_docs = docs;
    if (out_skipped) *out_skipped = skipped;
    return ORR_OK;
}

int orr_index_get_rows(orr_index *idx, int64_t n, const int64_t *row_ids, int32_t dim, float *out_emb, uint8_t *out_found)
{
    static const char *fn = "orr_index_get_rows";
    switch (centroid_index::first_invalid_get_rows(n, !row_ids, !out_emb, !idx)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: n is negative", fn);
    case 2: return fail(ORR_EINVAL, "%s: row_ids or out_emb is NULL with %lld entries", fn, (long long)n);
    default: return fail(ORR_EINVAL, "%s: null index", fn);
    }
    Lane ln = acquire_lane(idx);
    orr_index *lane = ln.lane;
    std::lock_guard<std::mutex> lock(lane->mu);
    if (!lane->sealed) return fail(ORR_ESTATE, "%s: the index is not sealed", fn);
    if (dim <= 0 || dim != lane->dim) return fail(ORR_EDIM, "%s: dim %d differs from the index dimension %d (and must be greater than 0)", fn, dim, lane->dim);
    if (n == 0) return ORR_OK;
    if (lane->n_rows <= 0) {
        memset(out_emb, 0, sizeof(float) * (size_t)n * (size_t)dim);
        if (out_found) memset(out_found, 0, (size_t)n);
        return ORR_OK;
    }
    ORR_TRY(bind_device(lane));
    ORR_TRY(ensure_scope_table(lane));
    const orr_index *own = owner_of(lane);
    hipStream_t s = lane->stream;
    const int64_t per = std::min<int64_t>(n, centroid_index::get_rows_slice(dim));
    DevBuf ids, pos, found, rows;
    auto body = [&]() -> int {
        ORR_TRY(ids.reserve(sizeof(int64_t) * (size_t)per));
        ORR_TRY(pos.reserve(sizeof(uint32_t) * (size_t)per));
        ORR_TRY(found.reserve((size_t)per));
        ORR_TRY(rows.reserve(sizeof(float) * (size_t)per * (size_t)dim));
        for (int64_t i0 = 0; i0 < n; i0 += per) {
            const int64_t c = std::min(per, n - i0);
            HIP_TRY(hipMemcpyAsync(ids.p, row_ids + i0, sizeof(int64_t) * (size_t)c, hipMemcpyHostToDevice, s));
            {
                Timed t(lane, "rows_find", 21.0 * (double)c);
                HIP_TRY(orr::launch_rows_find(own->scope_tab_ids, own->scope_tab_pos, lane->n_rows, ids.as<int64_t>(), c, own->d_dead.as<int64_t>(),
                                              (int32_t)own->dead.size(), pos.as<uint32_t>(), found.as<uint8_t>(), s));
            }
            {
                Timed t(lane, "rows_gather", 8.0 * (double)dim * (double)c);
                HIP_TRY(orr::launch_rows_gather(lane->d_emb, lane->n_rows, dim, pos.as<uint32_t>(), c, rows.as<float>(), s));
            }
            HIP_TRY(hipMemcpyAsync(out_emb + (size_t)i0 * (size_t)dim, rows.p, sizeof(float) * (size_t)c * (size_t)dim, hipMemcpyDeviceToHost, s));
            if (out_found) HIP_TRY(hipMemcpyAsync(out_found + i0, found.p, (size_t)c, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));          // (the workspace is the next slice's)
        }
        return ORR_OK;
    };
    const int r = body();
    (void)hipStreamSynchronize(s);
    collect_events(lane);
    for (DevBuf *b : {&ids, &pos, &found, &rows}) b->release();
    return r;
}

namespace {

// What a per-key call owns from its second round on: the frozen candidate set, the slice's exclusion bitmaps with their chunk
// counts, the union table, the seen pairs, the gather's staging.
struct PerKeyWork {
    DevBuf c_bm, ex_bm, ex_chunks, tab, seen, limits, gio;
    PinnedBuf pin;                                     // [live u32 x 64][took u32 x 64][clip i64 x 64]
    int64_t words = 0;
    bool frozen = false;
    std::vector<float> q_down;                         // device-resident queries come down once for the sub-batches
    ~PerKeyWork()
    {
        for (DevBuf *b : {&c_bm, &ex_bm, &ex_chunks, &tab, &seen, &limits, &gio}) b->release();
        pin.release();
    }
};

// out[i] = the key of position pos[i] (ORR_KEY_NONE for a negative one): ONE keys_gather launch, ends synchronised
int per_key_gather(orr_index *lane, const orr_keys *keys, DevBuf &io, const std::vector<int64_t> &pos, std::vector<int64_t> &out)
{
    const size_t n = pos.size();
    out.assign(n, ORR_KEY_NONE);
    if (n == 0) return ORR_OK;
    hipStream_t s = lane->stream;
    ORR_TRY(io.reserve(sizeof(int64_t) * 2 * n));
    int64_t *d_pos = io.as<int64_t>(), *d_out = d_pos + n;
    HIP_TRY(hipMemcpyAsync(d_pos, pos.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    {
        Timed t(lane, "keys_gather", 24.0 * (double)n);
        HIP_TRY(orr::launch_keys_gather(keys->d_key, lane->n_rows, d_pos, (int64_t)n, nullptr, nullptr, nullptr, 0, d_out, s));
    }
    HIP_TRY(hipMemcpyAsync(out.data(), d_out, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(lane);
    return ORR_OK;
}

// The frozen candidate set C of a call as a bitmap, built once when a second round is first needed: the rows that took part in
// round 1 -- `within`'s bits (or the live rows) below the clip position of the call's candidate_limit.  scope_took >= 0: the
// first scope_took rows of `within` instead (a cluster's shard: its share of the limit, orr_cluster_per_key_plan.h).
int per_key_freeze(orr_index *lane, const BatchArgs &a, const orr_scope *within, PerKeyWork &w, int64_t scope_took = -1)
{
    if (w.frozen) return ORR_OK;
    const orr_index *own = owner_of(lane);
    hipStream_t s = lane->stream;
    w.words = (int64_t)(scope::bitmap_bytes(lane->n_rows) / 4);
    ORR_TRY(w.c_bm.reserve(sizeof(uint32_t) * (size_t)w.words));
    int64_t n_clip = 0;
    if (!within) {
        n_clip = participating_rows(lane, a.candidate_limit);
    } else {
        const int64_t live = within->live.load(), took = scope_took >= 0 ? std::min<int64_t>(live, scope_took) : std::min<int64_t>(live, std::max<int64_t>(1, a.candidate_limit));
        n_clip = took > 0 ? within->n_clip_all : 0;
        if (took < live && took > 0) {
            ORR_TRY(lane->pin_mask.reserve(sizeof(int64_t)));
            {
                Timed t(lane, "mask_clip", 4.0 * (double)orr::kScopeChunkWords + 4.0 * (double)orr::scope_chunks(w.words));
                HIP_TRY(orr::launch_mask_clip(within->bm, within->words, within->chunks, (uint32_t)took, lane->pin_mask.as<int64_t>(), s));
            }
            HIP_TRY(hipStreamSynchronize(s));
            collect_events(lane);
            n_clip = *lane->pin_mask.as<int64_t>();
        }
    }
    n_clip = std::max<int64_t>(0, std::min<int64_t>(n_clip, lane->n_rows));
    {
        Timed t(lane, "scope_fill_range", 4.0 * (double)w.words);
        HIP_TRY(orr::launch_scope_fill_range(w.c_bm.as<uint32_t>(), w.words, 0, n_clip, s));
    }
    if (within) {
        Timed t(lane, "scope_combine", 12.0 * (double)w.words);
        HIP_TRY(orr::launch_scope_combine(w.c_bm.as<uint32_t>(), within->bm, w.words, ORR_SCOPE_AND, s));
    } else {
        Timed t(lane, "scope_clear_positions", 12.0 * (double)own->dead.size());
        HIP_TRY(orr::launch_scope_clear_positions(w.c_bm.as<uint32_t>(), w.words, own->d_dead.as<int64_t>(), (int64_t)own->dead.size(), s));
    }
    w.frozen = true;
    return ORR_OK;
}

int slice_scopes_reserve(int32_t S, int64_t words, PerKeyWork &w);
int slice_scopes_finish(orr_index *lane, int32_t S, PerKeyWork &w, std::unique_ptr<orr_scope[]> &tmp);
int per_key_slice_scopes(orr_index *lane, const orr_keys *keys, int32_t S, const std::vector<int64_t> &tk, const std::vector<uint64_t> &tm,
                         const std::vector<int64_t> &seen_pos, const std::vector<int32_t> &seen_slot, PerKeyWork &w, std::unique_ptr<orr_scope[]> &tmp);

// One round beyond the first for the unfinished queries `ids` (ascending, at most per_key::kMaxSlots) of the call `a` (vectors in
// host memory): ONE keys_exclude launch into the call's temporary scope bitmaps, at most one keys_clear_seen behind it, the
// counts the grouped stages ask of a scope, ONE search through grouped_batch (masked_batch for a slice of one query) over
// temporary scopes that are never registered with the index, and the round's rows with their positions: [ids.size()][pool].
int per_key_round(orr_index *lane, const BatchArgs &a, const orr_keys *keys, int32_t pool, const std::vector<int32_t> &ids,
                  const std::vector<per_key::State> &st, PerKeyWork &w, std::vector<int64_t> &r_rows, std::vector<double> &r_scores,
                  std::vector<int64_t> &r_pos, std::vector<int32_t> &r_cnt)
{
    const int32_t S = (int32_t)ids.size();
    // ---- the union table of the slots' closed keys, the seen pairs
    std::vector<const std::set<int64_t> *> closed((size_t)S);
    for (int32_t i = 0; i < S; ++i) closed[(size_t)i] = &st[(size_t)ids[(size_t)i]].closed;
    std::vector<int64_t> tk;
    std::vector<uint64_t> tm;
    per_key::build_table(closed, tk, tm);
    std::vector<int64_t> seen_pos;
    std::vector<int32_t> seen_slot;
    for (int32_t i = 0; i < S; ++i)
        for (int64_t p : st[(size_t)ids[(size_t)i]].seen) { seen_pos.push_back(p); seen_slot.push_back(i); }
    std::unique_ptr<orr_scope[]> tmp;
    ORR_TRY(per_key_slice_scopes(lane, keys, S, tk, tm, seen_pos, seen_slot, w, tmp));
    std::vector<const orr_scope *> ptrs((size_t)S);
    for (int32_t i = 0; i < S; ++i) ptrs[(size_t)i] = &tmp[(size_t)i];
    // ---- the search: C minus the exclusions, with no further limit
    SubBatch sb;
    BatchArgs cur;
    ORR_TRY(build_subset(lane, a, ids, sb, cur));
    cur.topk = pool;
    cur.candidate_limit = std::max<int64_t>(1, lane->n_rows);
    r_rows.assign((size_t)S * pool, -1); r_scores.assign((size_t)S * pool, 0.0); r_pos.assign((size_t)S * pool, -1); r_cnt.assign((size_t)S, 0);
    cur.out_keys = r_pos.data();
    lane->sstats.searches += 1;
    lane->sstats.queries += S;
    if (S == 1) {
        ORR_TRY(masked_batch(lane, cur, ScopeSource{nullptr, ptrs[0]}, r_rows.data(), r_scores.data(), r_cnt.data()));
    } else {
        std::vector<int32_t> qg((size_t)S);
        std::iota(qg.begin(), qg.end(), 0);
        GroupArgs ga{S, 0, nullptr, nullptr, qg.data()};
        ga.scopes = ptrs.data();
        ORR_TRY(grouped_batch(lane, cur, ga, r_rows.data(), r_scores.data(), r_cnt.data()));
    }
    return ORR_OK;
}

// The temporary scopes of a slice of S unfinished queries on one shard (the lane held, the frozen set built): the union table
// (tk, tm) of the slots' closed keys and the slots' seen positions (local to this shard) come to the device; ONE keys_exclude
// launch into the call's bitmaps, at most one keys_clear_seen behind it, the counts the grouped stages ask of a scope; one
// synchronise.  tmp[i]: slot i's scope, never registered with the index, valid while `w` is.
int per_key_slice_scopes(orr_index *lane, const orr_keys *keys, int32_t S, const std::vector<int64_t> &tk, const std::vector<uint64_t> &tm,
                         const std::vector<int64_t> &seen_pos, const std::vector<int32_t> &seen_slot, PerKeyWork &w, std::unique_ptr<orr_scope[]> &tmp)
{
    hipStream_t s = lane->stream;
    const int64_t words = w.words;
    const size_t n_tab = tk.size();
    const size_t n_seen = seen_pos.size();
    ORR_TRY(slice_scopes_reserve(S, words, w));
    ORR_TRY(w.tab.reserve(16 * std::max<size_t>(n_tab, 1)));
    ORR_TRY(w.seen.reserve(12 * std::max<size_t>(n_seen, 1)));
    int64_t *d_tk = w.tab.as<int64_t>();
    uint64_t *d_tm = reinterpret_cast<uint64_t *>(d_tk + n_tab);
    int64_t *d_seen_pos = w.seen.as<int64_t>();
    int32_t *d_seen_slot = reinterpret_cast<int32_t *>(d_seen_pos + n_seen);
    if (n_tab) {
        HIP_TRY(hipMemcpyAsync(d_tk, tk.data(), sizeof(int64_t) * n_tab, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_tm, tm.data(), sizeof(uint64_t) * n_tab, hipMemcpyHostToDevice, s));
    }
    if (n_seen) {
        HIP_TRY(hipMemcpyAsync(d_seen_pos, seen_pos.data(), sizeof(int64_t) * n_seen, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_seen_slot, seen_slot.data(), sizeof(int32_t) * n_seen, hipMemcpyHostToDevice, s));
    }
    uint32_t *ex = w.ex_bm.as<uint32_t>();
    {
        Timed t(lane, "keys_exclude", 8.0 * (double)lane->n_rows + 4.0 * (double)words * (double)(S + 1));
        HIP_TRY(orr::launch_keys_exclude(keys->d_key, lane->n_rows, w.c_bm.as<uint32_t>(), words, d_tk, d_tm, (int32_t)n_tab, S, ex, s));
    }
    if (n_seen) {
        Timed t(lane, "keys_clear_seen", 16.0 * (double)n_seen);
        HIP_TRY(orr::launch_keys_clear_seen(ex, words, S, d_seen_slot, d_seen_pos, (int64_t)n_seen, s));
    }
    return slice_scopes_finish(lane, S, w, tmp);
}

// The room a slice of S temporary scopes over `words` words takes in `w`: the bitmaps, their chunk counts, the limits, the
// pinned counts.
int slice_scopes_reserve(int32_t S, int64_t words, PerKeyWork &w)
{
    ORR_TRY(w.ex_bm.reserve(sizeof(uint32_t) * (size_t)S * (size_t)words));
    ORR_TRY(w.ex_chunks.reserve(sizeof(uint32_t) * (size_t)S * (size_t)orr::scope_chunks(words)));
    ORR_TRY(w.limits.reserve(sizeof(int64_t) * per_key::kMaxSlots + 2 * sizeof(uint32_t) * per_key::kMaxSlots));      // [limit][live][took]
    ORR_TRY(w.pin.reserve((4 + 4 + 8) * (size_t)per_key::kMaxSlots));
    return ORR_OK;
}

// What the S bitmaps in w.ex_bm (w.words words each, their launches queued on the lane's stream) still lack to be scopes the
// masked and grouped stages take: refresh_scope's two steps, each ONE launch for the S bitmaps (no limit: a scope keeps the
// count and the clip of ALL its rows; the stages apply the call's candidate_limit themselves), and one synchronise.
// tmp[i]: slot i's scope, never registered with the index, valid while `w` is.  Shared by the per-key rounds (keys_exclude)
// and the routed search (keys_include).
int slice_scopes_finish(orr_index *lane, int32_t S, PerKeyWork &w, std::unique_ptr<orr_scope[]> &tmp)
{
    hipStream_t s = lane->stream;
    const int64_t words = w.words;
    const int32_t n_chunks = orr::scope_chunks(words);
    uint32_t *ex = w.ex_bm.as<uint32_t>(), *exc = w.ex_chunks.as<uint32_t>();
    const std::vector<int64_t> no_limit((size_t)per_key::kMaxSlots, std::numeric_limits<int64_t>::max());
    HIP_TRY(hipMemcpyAsync(w.limits.p, no_limit.data(), sizeof(int64_t) * no_limit.size(), hipMemcpyHostToDevice, s));
    uint32_t *h_live = w.pin.as<uint32_t>();
    int64_t *h_clip = reinterpret_cast<int64_t *>(h_live + 2 * per_key::kMaxSlots);
    uint32_t *d_live = reinterpret_cast<uint32_t *>(w.limits.as<int64_t>() + per_key::kMaxSlots), *d_took = d_live + per_key::kMaxSlots;
    {
        Timed t(lane, "scope_counts", 4.0 * (double)S * (double)words);
        HIP_TRY(orr::launch_scope_counts(ex, words, S, S, w.limits.as<int64_t>(), exc, d_live, d_took, s));
    }
    {
        Timed t(lane, "mask_clip_slots", (4.0 * (double)orr::kScopeChunkWords + 4.0 * (double)n_chunks) * (double)S);
        HIP_TRY(orr::launch_mask_clip_slots(ex, words, exc, d_live, S, h_clip, s));
    }
    HIP_TRY(hipMemcpyAsync(h_live, d_live, sizeof(uint32_t) * (size_t)S, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    collect_events(lane);
    tmp.reset(new orr_scope[(size_t)S]);
    for (int32_t i = 0; i < S; ++i) {
        orr_scope &sc = tmp[(size_t)i];
        sc.owner.store(const_cast<orr_index *>(owner_of(lane)));
        sc.n_rows = lane->n_rows; sc.words = words;
        sc.bm = ex + (size_t)i * (size_t)words; sc.chunks = exc + (size_t)i * (size_t)n_chunks;
        sc.live.store((int64_t)h_live[i]);
        sc.n_clip_all = std::min<int64_t>(h_clip[i], lane->n_rows);
    }
    return ORR_OK;
}

// orr_search_batch_per_key on the lane the caller holds (the scope, if any, and the keys held shared).
int per_key_run(orr_index *lane, const char *fn, const BatchArgs &a, const orr_scope *within, const orr_keys *keys, int32_t max_per_key,
                int32_t pool, int64_t *out_rows, double *out_scores, int64_t *out_row_keys, int32_t *out_counts, int32_t *out_rounds)
{
    const int32_t B = a.B, take = per_key::take_of(a.topk);
    for (size_t i = 0; i < (size_t)B * take; ++i) { out_rows[i] = -1; out_scores[i] = 0.0; out_row_keys[i] = ORR_KEY_NONE; }
    for (int32_t b = 0; b < B; ++b) { out_counts[b] = 0; if (out_rounds) out_rounds[b] = 0; }
    // ---- round 1: the pool, exactly the call the diverse search makes for its own
    std::vector<int64_t> r_rows((size_t)B * pool, -1), r_pos((size_t)B * pool, -1);
    std::vector<double> r_scores((size_t)B * pool, 0.0);
    std::vector<int32_t> r_cnt((size_t)B, 0);
    {
        BatchArgs pa = a;
        pa.topk = pool;
        pa.out_keys = r_pos.data();
        if (within) {
            ORR_TRY(masked_batch(lane, pa, ScopeSource{nullptr, within}, r_rows.data(), r_scores.data(), r_cnt.data()));
        } else {
            const int64_t n = participating_rows(lane, a.candidate_limit);
            ORR_TRY(escalate(index_backend(lane, fn, n), pa, escalation::initial_kprime(pool, n, orr::kSelWidth), r_rows.data(), r_scores.data(), r_cnt.data()));
        }
    }
    ORR_TRY(bind_device(lane));
    PerKeyWork w;
    std::vector<per_key::State> st((size_t)B);
    std::vector<int32_t> ids((size_t)B);               // the queries of the round in flight: [i] of r_* is query ids[i]
    std::iota(ids.begin(), ids.end(), 0);
    std::vector<int64_t> kept_rows, kept_keys;         // [B][take], filled as the walks keep rows
    std::vector<double> kept_scores;
    BatchArgs host_a = a;
    for (int32_t round = 1; !ids.empty(); ++round) {
        if (round > take) return fail(ORR_EDEVICE, "%s: a round kept no row", fn);      // (every round keeps at least one)
        // ---- the round's keys: ONE keys_gather
        const size_t nq = ids.size();
        std::vector<int64_t> pos(nq * (size_t)pool, -1), rk;
        for (size_t i = 0; i < nq; ++i)
            for (int32_t j = 0; j < r_cnt[i]; ++j) {
                const int64_t p = r_pos[i * pool + j] - lane->row_base;
                if (p < 0 || p >= lane->n_rows) return fail(ORR_EDEVICE, "%s: a result's order_key lies outside the shard", fn);
                pos[i * pool + j] = p;
            }
        ORR_TRY(per_key_gather(lane, keys, w.gio, pos, rk));
        // ---- the walk
        std::vector<int32_t> unfinished;
        std::vector<int32_t> number((size_t)pool);
        std::iota(number.begin(), number.end(), 0);
        for (size_t i = 0; i < nq; ++i) {
            const int32_t b = ids[i];
            per_key::State &s = st[(size_t)b];
            const size_t had = s.kept.size();
            per_key::walk_round(s, r_cnt[i], rk.data() + i * pool, pos.data() + i * pool, number.data(), take, max_per_key, pool);
            for (size_t t = had; t < s.kept.size(); ++t) {
                const size_t o = (size_t)b * take + t, from = i * pool + (size_t)s.kept[t];
                out_rows[o] = r_rows[from]; out_scores[o] = r_scores[from]; out_row_keys[o] = rk[from];
            }
            out_counts[b] = (int32_t)s.kept.size();
            if (out_rounds) out_rounds[b] = s.rounds;
            if (!s.finished) {
                if (s.kept.size() == had) return fail(ORR_EDEVICE, "%s: a round kept no row", fn);
                unfinished.push_back(b);
            }
        }
        if (unfinished.empty()) break;
        // ---- the next round, in slices of at most 64 queries
        if (!w.frozen) {
            ORR_TRY(per_key_freeze(lane, a, within, w));
            if (a.dim > 0 && is_device_pointer(a.q)) {
                w.q_down.resize((size_t)B * (size_t)a.dim);
                HIP_TRY(hipMemcpy(w.q_down.data(), a.q, sizeof(float) * w.q_down.size(), hipMemcpyDeviceToHost));
                host_a.q = w.q_down.data();
            }
        }
        const size_t nu = unfinished.size();
        std::vector<int64_t> n_rows(nu * (size_t)pool, -1), n_pos(nu * (size_t)pool, -1);
        std::vector<double> n_scores(nu * (size_t)pool, 0.0);
        std::vector<int32_t> n_cnt(nu, 0);
        for (size_t b0 = 0; b0 < nu; b0 += (size_t)per_key::kMaxSlots) {
            const size_t S = std::min<size_t>((size_t)per_key::kMaxSlots, nu - b0);
            const std::vector<int32_t> slice(unfinished.begin() + b0, unfinished.begin() + b0 + S);
            std::vector<int64_t> s_rows, s_pos;
            std::vector<double> s_scores;
            std::vector<int32_t> s_cnt;
            ORR_TRY(per_key_round(lane, host_a, keys, pool, slice, st, w, s_rows, s_scores, s_pos, s_cnt));
            memcpy(n_rows.data() + b0 * pool, s_rows.data(), sizeof(int64_t) * S * pool);
            memcpy(n_pos.data() + b0 * pool, s_pos.data(), sizeof(int64_t) * S * pool);
            memcpy(n_scores.data() + b0 * pool, s_scores.data(), sizeof(double) * S * pool);
            memcpy(n_cnt.data() + b0, s_cnt.data(), sizeof(int32_t) * S);
        }
        ids.swap(unfinished);
        r_rows.swap(n_rows); r_pos.swap(n_pos); r_scores.swap(n_scores); r_cnt.swap(n_cnt);
    }
    return ORR_OK;
}

}  // namespace

int orr_search_batch_per_key(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8, const uint32_t *term_off,
                             const uint32_t *query_term_off, int64_t now_ticks, int32_t topk, int64_t candidate_limit, const orr_scope *within,
                             const orr_keys *keys, int32_t max_per_key, int32_t pool, int64_t *out_rows, double *out_scores, int64_t *out_keys,
                             int32_t *out_counts, int32_t *out_rounds)
{
    static const char *fn = "orr_search_batch_per_key";
    switch (per_key::first_invalid(!out_rows || !out_scores || !out_keys || !out_counts, topk, pool, max_per_key, !keys)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out_rows, out_scores, out_keys and out_counts are required", fn);
    case 2: return fail(ORR_EINVAL, "%s: pool must be in 1 .. %d", fn, per_key::kMaxPool);
    case 3: return fail(ORR_EINVAL, "%s: topk %d exceeds the pool of %d", fn, topk, pool);
    case 4: return fail(ORR_EINVAL, "%s: max_per_key must be at least 1", fn);
    default: return fail(ORR_EINVAL, "%s: null keys", fn);
    }
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    if (B == 0) return ORR_OK;
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    ORR_TRY(check_batch(idx, a, fn));
    orr_index *own = nullptr;
    if (within) ORR_TRY(scope_owner(within, idx, fn, &own));
    ORR_TRY(keys_owner(keys, idx, fn, &own));
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    std::shared_lock<std::shared_mutex> rd;
    if (within) {
        rd = std::shared_lock<std::shared_mutex>(within->mu);
        ORR_TRY(scope_owner(within, idx, fn, &own));
        if (within->n_rows != idx->n_rows) return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)within->n_rows, (long long)idx->n_rows);
    }
    std::shared_lock<std::shared_mutex> rk(keys->mu);
    ORR_TRY(keys_owner(keys, idx, fn, &own));
    if (keys->n_rows != idx->n_rows) return fail(ORR_ESTATE, "%s: the keys cover %lld rows, the handle %lld", fn, (long long)keys->n_rows, (long long)idx->n_rows);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    const int r = per_key_run(idx, fn, a, within, keys, max_per_key, pool, out_rows, out_scores, out_keys, out_counts, out_rounds);
    g_ht.done();
    return r;
}

// ---- routed search (orr_search_batch_routed; the rules are orr_routed_plan.h's) -----------------------------------------------
// The route step is the public orr_search_batch on `docs`; the chunk step reuses the per-key rounds' machinery with the opposite
// kernel: per slice of at most 64 distinct routes ONE keys_include launch into temporary bitmaps, slice_scopes_finish, ONE
// grouped_batch (masked_batch for a slice of one slot) over temporary scopes that are never registered with the index.

namespace {

// The chunk step on the lane the caller holds (keys and `within`, if any, held shared): route_keys [B][route] and route_n [B] are
// the route step's answer; rows / scores [B][take] and counts [B] receive the call's.
int routed_run(orr_index *lane, const BatchArgs &a, const orr_keys *keys, const orr_scope *within, int32_t route, const int64_t *route_keys,
               const int32_t *route_n, int64_t *rows, double *scores, int32_t *counts)
{
    const int32_t B = a.B, take = std::max<int32_t>(1, a.topk);
    for (size_t i = 0; i < (size_t)B * take; ++i) { rows[i] = -1; scores[i] = 0.0; }
    for (int32_t b = 0; b < B; ++b) counts[b] = 0;
    if (lane->n_rows <= 0 || (within && within->live.load() <= 0)) return ORR_OK;
    const routed::Slots slots = routed::slots(B, route, route_keys, route_n);
    const std::vector<routed::Slice> slices = routed::slices(slots);
    if (slices.empty()) return ORR_OK;                 // no query routed anywhere: nothing is launched
    ORR_TRY(bind_device(lane));
    hipStream_t s = lane->stream;
    PerKeyWork w;
    // ---- the base the in-scope twin would AND with: `within`'s bitmap where it lies, or the live rows
    const uint32_t *base = nullptr;
    if (within) {
        w.words = within->words;
        base = within->bm;
    } else {
        BatchArgs all = a;
        all.candidate_limit = lane->row_base + lane->n_rows;           // every row of the shard
        ORR_TRY(per_key_freeze(lane, all, nullptr, w));
        base = w.c_bm.as<uint32_t>();
    }
    const int64_t words = w.words;
    BatchArgs host_a = a;
    if (a.dim > 0 && is_device_pointer(a.q)) {         // (sub-batches are gathered on the host: device-resident vectors come down once)
        w.q_down.resize((size_t)B * (size_t)a.dim);
        HIP_TRY(hipMemcpy(w.q_down.data(), a.q, sizeof(float) * w.q_down.size(), hipMemcpyDeviceToHost));
        host_a.q = w.q_down.data();
    }
    std::vector<int64_t> tk, s_rows;
    std::vector<uint64_t> tm;
    std::vector<double> s_scores;
    std::vector<int32_t> s_cnt;
    for (const routed::Slice &c : slices) {
        const int32_t S = c.n_slots;
        routed::slice_table(slots, c, tk, tm);
        const size_t n_tab = tk.size();
        ORR_TRY(slice_scopes_reserve(S, words, w));
        ORR_TRY(w.tab.reserve(16 * std::max<size_t>(n_tab, 1)));
        int64_t *d_tk = w.tab.as<int64_t>();
        uint64_t *d_tm = reinterpret_cast<uint64_t *>(d_tk + n_tab);
        HIP_TRY(hipMemcpyAsync(d_tk, tk.data(), sizeof(int64_t) * n_tab, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_tm, tm.data(), sizeof(uint64_t) * n_tab, hipMemcpyHostToDevice, s));
        {
            // the keys, every word of the S bitmaps written; the base words of the workgroups that hold a routed row are read too,
            // but how many those are only the device knows: they are not counted
            Timed t(lane, "keys_include", 8.0 * (double)lane->n_rows + 4.0 * (double)words * (double)S);
            HIP_TRY(orr::launch_keys_include(keys->d_key, lane->n_rows, base, words, d_tk, d_tm, (int32_t)n_tab, S, w.ex_bm.as<uint32_t>(), s));
        }
        std::unique_ptr<orr_scope[]> tmp;
        ORR_TRY(slice_scopes_finish(lane, S, w, tmp));
        std::vector<const orr_scope *> ptrs((size_t)S);
        for (int32_t i = 0; i < S; ++i) ptrs[(size_t)i] = &tmp[(size_t)i];
        // ---- the search: every query inside its slot's scope, the call's own topk and candidate_limit
        const size_t nq = c.queries.size();
        SubBatch sb;
        BatchArgs cur;
        ORR_TRY(build_subset(lane, host_a, c.queries, sb, cur));
        s_rows.assign(nq * (size_t)take, -1); s_scores.assign(nq * (size_t)take, 0.0); s_cnt.assign(nq, 0);
        if (S == 1) {
            ORR_TRY(masked_batch(lane, cur, ScopeSource{nullptr, ptrs[0]}, s_rows.data(), s_scores.data(), s_cnt.data()));
        } else {
            GroupArgs ga{S, 0, nullptr, nullptr, c.query_slot.data()};
            ga.scopes = ptrs.data();
            ORR_TRY(grouped_batch(lane, cur, ga, s_rows.data(), s_scores.data(), s_cnt.data()));
        }
        for (size_t i = 0; i < nq; ++i) {
            const size_t b = (size_t)c.queries[i];
            memcpy(rows + b * take, s_rows.data() + i * take, sizeof(int64_t) * (size_t)take);
            memcpy(scores + b * take, s_scores.data() + i * take, sizeof(double) * (size_t)take);
            counts[b] = s_cnt[i];
        }
    }
    return ORR_OK;
}

}  // namespace

int orr_search_batch_routed(orr_index *docs, orr_index *idx, const orr_keys *keys, int32_t B, int32_t dim, const float *q,
                            const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks,
                            int32_t route, int32_t topk, int64_t candidate_limit, const orr_scope *within, int64_t *out_rows,
                            double *out_scores, int32_t *out_counts, int64_t *out_route_keys, int32_t *out_route_n)
{
    static const char *fn = "orr_search_batch_routed";
    switch (routed::first_invalid(!out_rows || !out_scores || !out_counts, route, !keys, !docs)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out_rows, out_scores and out_counts are required", fn);
    case 2: return fail(ORR_EINVAL, "%s: route must be in 1 .. %d", fn, routed::kMaxRoute);
    case 3: return fail(ORR_EINVAL, "%s: null keys", fn);
    default: return fail(ORR_EINVAL, "%s: null document index", fn);
    }
    if (!idx) return fail(ORR_EINVAL, "%s: null index", fn);
    if (B == 0) return ORR_OK;
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    ORR_TRY(check_batch(idx, a, fn));
    orr_index *own = nullptr;
    if (within) ORR_TRY(scope_owner(within, idx, fn, &own));
    ORR_TRY(keys_owner(keys, idx, fn, &own));
    // ---- route: the public search on docs, its own lane taken and released before a lane of idx is (docs may be idx)
    const int32_t take = std::max<int32_t>(1, topk);
    std::vector<int64_t> r_keys((size_t)B * (size_t)route, ORR_KEY_NONE);
    std::vector<double> r_scores((size_t)B * (size_t)route, 0.0);
    std::vector<int32_t> r_n((size_t)B, 0);
    ORR_TRY(orr_search_batch(docs, B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, route, std::max<int64_t>(1, orr_index_rows(docs)),
                             r_keys.data(), r_scores.data(), r_n.data()));
    for (int32_t b = 0; b < B; ++b)                     // (a row id may be any key, -1 included: the count tells what was returned)
        for (int32_t j = std::max<int32_t>(0, r_n[(size_t)b]); j < route; ++j) r_keys[(size_t)b * route + j] = ORR_KEY_NONE;
    // ---- chunks: one lane of idx, the scope first, then the keys, as orr_search_batch_per_key
    std::vector<int64_t> rows((size_t)B * (size_t)take);
    std::vector<double> scores((size_t)B * (size_t)take);
    std::vector<int32_t> counts((size_t)B);
    {
        Lane ln = acquire_lane(idx);
        orr_index *lane = ln.lane;
        std::lock_guard<std::mutex> lock(lane->mu);
        std::shared_lock<std::shared_mutex> rd;
        if (within) {
            rd = std::shared_lock<std::shared_mutex>(within->mu);
            ORR_TRY(scope_owner(within, lane, fn, &own));
            if (within->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)within->n_rows, (long long)lane->n_rows);
        }
        std::shared_lock<std::shared_mutex> rk(keys->mu);
        ORR_TRY(keys_owner(keys, lane, fn, &own));
        if (keys->n_rows != lane->n_rows) return fail(ORR_ESTATE, "%s: the keys cover %lld rows, the handle %lld", fn, (long long)keys->n_rows, (long long)lane->n_rows);
        lane->sstats.searches += 1;                    // as one grouped call
        lane->sstats.queries += B;
        const int r = routed_run(lane, a, keys, within, route, r_keys.data(), r_n.data(), rows.data(), scores.data(), counts.data());
        g_ht.done();
        if (r != ORR_OK) return r;
    }
    memcpy(out_rows, rows.data(), sizeof(int64_t) * rows.size());
    memcpy(out_scores, scores.data(), sizeof(double) * scores.size());
    memcpy(out_counts, counts.data(), sizeof(int32_t) * counts.size());
    if (out_route_keys) memcpy(out_route_keys, r_keys.data(), sizeof(int64_t) * r_keys.size());
    if (out_route_n) memcpy(out_route_n, r_n.data(), sizeof(int32_t) * r_n.size());
    return ORR_OK;
}

int orr_search_shard_scoped(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                            const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                            int64_t candidate_limit, int32_t topk, int64_t n_scope_ids, const int64_t *scope_ids,
                            const uint64_t *scope_off, const int64_t *scope_before, orr_candidate *out)
{
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, kprime};
    const ScopeArgs sc{n_scope_ids, scope_ids, scope_off, scope_before};
    ORR_TRY(check_scope(idx, B, sc, "orr_search_shard_scoped"));
    ORR_TRY(check_batch(idx, a, "orr_search_shard_scoped"));
    if (kprime < 1) return fail(ORR_EINVAL, "orr_search_shard_scoped: kprime must be >= 1");
    if (topk < 0) return fail(ORR_EINVAL, "orr_search_shard_scoped: topk must be >= 0");
    if (!out) return fail(ORR_EINVAL, "orr_search_shard_scoped: out is NULL");
    if (topk > 0) a.topk = std::min<int32_t>(kprime, topk);
    Lane ln = acquire_lane(idx);
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return scoped_shard(idx, a, sc, kprime, out);
}

int orr_index_scope_count(orr_index *idx, int32_t B, int64_t n_scope_ids, const int64_t *scope_ids, const uint64_t *scope_off,
                          int64_t *out_live)
{
    const ScopeArgs sc{n_scope_ids, scope_ids, scope_off, nullptr};
    ORR_TRY(check_scope(idx, B, sc, "orr_index_scope_count"));
    if (B <= 0) return fail(ORR_EINVAL, "orr_index_scope_count: batch size must be positive");
    if (!out_live) return fail(ORR_EINVAL, "orr_index_scope_count: out_live is NULL");
    if (!idx->sealed) return fail(ORR_ESTATE, "orr_index_scope_count: index is not sealed");
    Lane ln = acquire_lane(idx);
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    return scope_count_on_lane(idx, B, sc, out_live);
}

int orr_search_shard_masked(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                            const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                            int64_t candidate_limit, int32_t topk, int32_t pass, int64_t n_scope_ids, const int64_t *scope_ids,
                            int64_t scope_before, orr_candidate *out)
{
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, kprime};
    const ScopeArgs sc{n_scope_ids, scope_ids, nullptr, nullptr};
    if (kprime < 1) return fail(ORR_EINVAL, "orr_search_shard_masked: kprime must be >= 1");
    if (topk < 0) return fail(ORR_EINVAL, "orr_search_shard_masked: topk must be >= 0");
    if (pass < 0 || pass > 1) return fail(ORR_EINVAL, "orr_search_shard_masked: pass takes 0 (the library's choice) or 1 (the list path)");
    if (scope_before < 0) return fail(ORR_EINVAL, "orr_search_shard_masked: scope_before is negative");
    if (!out) return fail(ORR_EINVAL, "orr_search_shard_masked: out is NULL");
    ORR_TRY(check_scope(idx, B, sc, "orr_search_shard_masked"));
    ORR_TRY(check_batch(idx, a, "orr_search_shard_masked"));
    if (topk > 0) a.topk = std::min<int32_t>(kprime, topk);
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return masked_shard(idx, a, ScopeSource{&sc, nullptr}, scope_before, kprime, pass, out);
}

int orr_search_shard_in_scope(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                              const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                              int64_t candidate_limit, int32_t topk, int32_t pass, const orr_scope *scope, int64_t scope_before,
                              orr_candidate *out)
{
    static const char *fn = "orr_search_shard_in_scope";
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, kprime};
    if (kprime < 1) return fail(ORR_EINVAL, "%s: kprime must be >= 1", fn);
    if (topk < 0) return fail(ORR_EINVAL, "%s: topk must be >= 0", fn);
    if (pass < 0 || pass > 1) return fail(ORR_EINVAL, "%s: pass takes 0 (the library's choice) or 1 (the list path)", fn);
    if (scope_before < 0) return fail(ORR_EINVAL, "%s: scope_before is negative", fn);
    if (!out) return fail(ORR_EINVAL, "%s: out is NULL", fn);
    if (!scope) return fail(ORR_EINVAL, "%s: null scope", fn);
    ORR_TRY(check_batch(idx, a, fn));
    if (topk > 0) a.topk = std::min<int32_t>(kprime, topk);
    orr_index *own = nullptr;
    ORR_TRY(scope_owner(scope, idx, fn, &own));
    Lane ln = acquire_lane(idx);                       // a search like any other: its own lane, concurrent with the others
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    std::shared_lock<std::shared_mutex> rd(scope->mu);
    ORR_TRY(scope_owner(scope, idx, fn, &own));
    if (scope->n_rows != idx->n_rows) return fail(ORR_ESTATE, "%s: the scope covers %lld rows, the handle %lld", fn, (long long)scope->n_rows, (long long)idx->n_rows);
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return masked_shard(idx, a, ScopeSource{nullptr, scope}, scope_before, kprime, pass, out);
}

int orr_search_shard_in_scopes(orr_index *idx, int32_t B, int32_t dim, const float *q, const uint8_t *terms_utf8,
                               const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                               int64_t candidate_limit, int32_t topk, int32_t pass, int32_t n_scopes, const orr_scope *const *scopes,
                               const int32_t *query_scope, const int64_t *scope_before, orr_candidate *out)
{
    static const char *fn = "orr_search_shard_in_scopes";
    BatchArgs a{B, dim, q, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, kprime};
    if (!scope_set::scopes_valid(n_scopes)) return fail(ORR_EINVAL, "%s: n_scopes must be in 1 .. %d", fn, scope_set::kMaxScopes);
    if (!scopes) return fail(ORR_EINVAL, "%s: scopes is NULL", fn);
    for (int32_t g = 0; g < n_scopes; ++g)
        if (!scopes[g]) return fail(ORR_EINVAL, "%s: scopes[%d] is a null scope", fn, g);
    if (!query_scope) return fail(ORR_EINVAL, "%s: query_scope is NULL", fn);
    if (B > 0 && !group::assignment_valid(query_scope, B, n_scopes))
        return fail(ORR_EINVAL, "%s: query_scope must name a scope in 0 .. %d for every query", fn, n_scopes - 1);
    if (!scope_before) return fail(ORR_EINVAL, "%s: scope_before is NULL", fn);
    for (int32_t g = 0; g < n_scopes; ++g)
        if (scope_before[g] < 0) return fail(ORR_EINVAL, "%s: scope_before[%d] is negative", fn, g);
    if (kprime < 1) return fail(ORR_EINVAL, "%s: kprime must be >= 1", fn);
    if (topk < 0) return fail(ORR_EINVAL, "%s: topk must be >= 0", fn);
    if (pass < 0 || pass > 1) return fail(ORR_EINVAL, "%s: pass takes 0 (the library's choice) or 1 (the list path)", fn);
    if (!out) return fail(ORR_EINVAL, "%s: out is NULL", fn);
    ORR_TRY(check_batch(idx, a, fn));
    if (topk > 0) a.topk = std::min<int32_t>(kprime, topk);
    orr_index *own = nullptr;
    for (int32_t g = 0; g < n_scopes; ++g) ORR_TRY(scope_owner(scopes[g], idx, fn, &own));
    Lane ln = acquire_lane(idx);
    idx = ln.lane;
    std::lock_guard<std::mutex> lock(idx->mu);
    // every distinct scope shared, in address order
    std::vector<const orr_scope *> distinct(scopes, scopes + n_scopes);
    std::sort(distinct.begin(), distinct.end(), std::less<const orr_scope *>());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    std::vector<std::shared_lock<std::shared_mutex>> held;
    held.reserve(distinct.size());
    for (const orr_scope *sc : distinct) held.emplace_back(sc->mu);
    for (const orr_scope *sc : distinct) {
        ORR_TRY(scope_owner(sc, idx, fn, &own));
        if (sc->n_rows != idx->n_rows) return fail(ORR_ESTATE, "%s: a scope covers %lld rows, the handle %lld", fn, (long long)sc->n_rows, (long long)idx->n_rows);
    }
    GroupArgs ga{n_scopes, 0, nullptr, nullptr, query_scope};
    ga.scopes = scopes;
    idx->sstats.searches += 1;
    idx->sstats.queries += B;
    return grouped_shard(idx, a, ga, scope_before, kprime, pass, out, nullptr);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// orr_cluster: several shards behind ONE handle in ONE process (the reference host is a single process: Program.cs:59,
// IngestionServiceCollectionExtensions.cs:22-23).  Shard i lives on devices[i] and holds a contiguous range of the global
// candidate order (rows of shard i are all at least as new as those of shard i + 1).  A search runs orr_search_shard's
// device side on every shard at once (one host thread per shard, each bound to its device), the [B][k'+1] records of
// every shard come back through pinned host memory, and the host finishes all queries exactly as orr_merge_candidates
// does -- the record exchange of the multi-process path (RCCL all-gather, sharded.py) without the collective, because
// here every record is wanted in ONE address space.  Escalation is per query, as in orr_search_batch.
// ---------------------------------------------------------------------------------------------------------------------
// RCCL, bound at run time (dlopen: the library stays loadable without it, and the default record exchange does not use it).
// Declarations as in <rccl/rccl.h> (NCCL-compatible ABI): opaque communicator, int result (0 = success), ncclInt8 = 0.
struct RcclApi {
    void *lib = nullptr;
    int (*CommInitAll)(void **comms, int ndev, const int *devlist) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    int (*AllGather)(const void *send, void *recv, size_t count, int dtype, void *comm, hipStream_t stream) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    static RcclApi *get()
    {
        static RcclApi *api = [] {
            RcclApi *a = new RcclApi();
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                a->lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
                if (a->lib) break;
            }
            if (!a->lib) return a;
            a->CommInitAll = reinterpret_cast<decltype(a->CommInitAll)>(dlsym(a->lib, "ncclCommInitAll"));
            a->CommDestroy = reinterpret_cast<decltype(a->CommDestroy)>(dlsym(a->lib, "ncclCommDestroy"));
            a->AllGather = reinterpret_cast<decltype(a->AllGather)>(dlsym(a->lib, "ncclAllGather"));
            a->GroupStart = reinterpret_cast<decltype(a->GroupStart)>(dlsym(a->lib, "ncclGroupStart"));
            a->GroupEnd = reinterpret_cast<decltype(a->GroupEnd)>(dlsym(a->lib, "ncclGroupEnd"));
            a->GetErrorString = reinterpret_cast<decltype(a->GetErrorString)>(dlsym(a->lib, "ncclGetErrorString"));
            return a;
        }();
        return api;
    }
    bool ok() const { return lib && CommInitAll && CommDestroy && AllGather && GroupStart && GroupEnd; }
    const char *text(int r) const { return GetErrorString ? GetErrorString(r) : "RCCL error"; }
};

struct orr_cluster {
    std::vector<orr_index *> shards;
    int32_t dim = 0;
    bool sealed = false;
    std::shared_mutex mu;              // searches share it (they run side by side, each shard search on a lane of its shard); seal / destroy take it alone
    std::mutex stats_mu;
    orr_search_stats sstats{};
    // optional record exchange over RCCL ("exchange" = 1): one communicator per shard device, one all-gather of the per-shard
    // [B][k'+1] records on the shards' exchange streams, the merge reads device 0's gathered copy.  One exchange at a time.
    int exchange = 0;                  // 0: pinned host memory (default); 1: RCCL all-gather over xGMI
    std::mutex rccl_mu;
    std::vector<void *> comms;         // [G], created at the first exchange
    std::vector<hipStream_t> xstreams; // [G]
    std::vector<DevBuf> xsend, xrecv;  // [G] grow-only
    PinnedBuf xhost;
    int64_t rccl_exchanges = 0;        // all-gathers done (orr_cluster_search_stats reports them in reserved[0])
    std::vector<orr_cluster_scope *> cscopes;   // cluster scope handles that are alive, under g_scope_life_mu: orr_cluster_destroy orphans them
    std::vector<orr_cluster_keys *> ckeys;      // cluster keys handles, likewise
};

// A cluster scope handle: one orr_scope per shard of one sealed cluster, each made on its shard and registered there, so the
// shards' maintenance carries them.  No count is kept here: rows and the search read every part's live when they are called.
struct orr_cluster_scope {
    std::atomic<orr_cluster *> owner{nullptr};   // nullptr: orphaned (the cluster was destroyed, or an edit ended on some shards only)
    std::vector<orr_scope *> parts;              // [shards]
};

// A cluster keys handle: one orr_keys per shard of one sealed cluster, each made on its shard and registered there
// (orr_index::key_cols), so the shards' maintenance carries them.
struct orr_cluster_keys {
    std::atomic<orr_cluster *> owner{nullptr};   // nullptr: orphaned (the cluster was destroyed, or an edit ended on some shards only)
    std::vector<orr_keys *> parts;               // [shards]
};

namespace {

// Persistent host threads for the shard halves of cluster searches: a search hands shards 1.. to the pool and runs shard 0
// itself (round 2 started G - 1 threads per call).  The pool grows with demand (concurrent searches each need G - 1 workers)
// up to a cap; its threads sleep between tasks and live as long as the process.
class ShardPool {
public:
    static ShardPool &get() { static ShardPool *p = new ShardPool(); return *p; }
    void submit(std::function<void()> task)
    {
        std::unique_lock<std::mutex> l(mu_);
        queue_.push_back(std::move(task));
        if (idle_ == 0 && (int)threads_ < kMaxThreads && !forked_.load(std::memory_order_relaxed)) {
            ++threads_;
            std::thread([this] { loop(); }).detach();
        }
        l.unlock();
        cv_.notify_one();
    }
    bool usable() const { return !forked_.load(std::memory_order_relaxed); }

private:
    static constexpr int kMaxThreads = 128;
    ShardPool() { pthread_atfork(nullptr, nullptr, [] { forked_.store(true); }); }
    void loop()
    {
        std::unique_lock<std::mutex> l(mu_);
        for (;;) {
            ++idle_;
            cv_.wait(l, [this] { return !queue_.empty(); });
            --idle_;
            std::function<void()> task = std::move(queue_.front());
            queue_.pop_front();
            l.unlock();
            task();
            l.lock();
        }
    }
    static inline std::atomic<bool> forked_{false};
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> queue_;
    int idle_ = 0;
    unsigned threads_ = 0;
};

// fn(i) for every shard at once (the calling thread takes shard 0, pool threads the others); returns the first failure
int for_each_shard(int32_t n, const std::function<int(int32_t)> &fn)
{
    std::vector<int> rc((size_t)n, ORR_OK);
    std::vector<std::string> msg((size_t)n);
    std::mutex done_mu;
    std::condition_variable done_cv;
    int pending = 0;
    const bool pooled = ShardPool::get().usable();
    for (int32_t i = 1; i < n; ++i) {
        auto task = [&, i] {
            rc[(size_t)i] = fn(i);
            if (rc[(size_t)i] != ORR_OK) msg[(size_t)i] = g_last_error;
            std::lock_guard<std::mutex> l(done_mu);
            if (--pending == 0) done_cv.notify_one();
        };
        {
            std::lock_guard<std::mutex> l(done_mu);
            ++pending;
        }
        if (pooled) ShardPool::get().submit(task);
        else task();
    }
    rc[0] = fn(0);
    if (rc[0] != ORR_OK) msg[0] = g_last_error;
    {
        std::unique_lock<std::mutex> l(done_mu);
        done_cv.wait(l, [&] { return pending == 0; });
    }
    for (int32_t i = 0; i < n; ++i)
        if (rc[(size_t)i] != ORR_OK) { g_last_error = msg[(size_t)i]; return rc[(size_t)i]; }     // (the detail was set on that shard's thread)
    return ORR_OK;
}

// Communicators, exchange streams and buffers of a cluster's RCCL record exchange (caller holds c->rccl_mu).  Any failure
// switches the cluster back to the pinned-host exchange for good and says why in orr_last_error().
int rccl_prepare(orr_cluster *c, size_t bytes_per_shard)
{
    const int G = (int)c->shards.size();
    RcclApi *api = RcclApi::get();
    auto give_up = [&](const char *why, const char *detail) {
        c->exchange = 0;
        return fail(ORR_ECOMM, "orr_cluster: RCCL exchange disabled (%s%s%s); records travel through pinned host memory", why, detail ? ": " : "", detail ? detail : "");
    };
    if (!api->ok()) return give_up("librccl.so could not be loaded", dlerror());
    if (c->comms.empty()) {
        std::vector<int> devs((size_t)G);
        for (int g = 0; g < G; ++g) {
            devs[(size_t)g] = c->shards[(size_t)g]->device;
            for (int h = 0; h < g; ++h)
                if (devs[(size_t)h] == devs[(size_t)g]) return give_up("two shards share a device, a communicator needs distinct ones", nullptr);
        }
        std::vector<void *> comms((size_t)G, nullptr);
        const int r = api->CommInitAll(comms.data(), G, devs.data());
        if (r != 0) return give_up("ncclCommInitAll failed", api->text(r));
        c->comms = comms;
        c->xstreams.assign((size_t)G, nullptr);
        c->xsend.resize((size_t)G);
        c->xrecv.resize((size_t)G);
        for (int g = 0; g < G; ++g) {
            if (hipSetDevice(devs[(size_t)g]) != hipSuccess || hipStreamCreateWithFlags(&c->xstreams[(size_t)g], hipStreamNonBlocking) != hipSuccess)
                return give_up("cannot create an exchange stream", nullptr);
        }
    }
    for (int g = 0; g < G; ++g) {
        if (hipSetDevice(c->shards[(size_t)g]->device) != hipSuccess) return give_up("hipSetDevice failed", nullptr);
        if (c->xsend[(size_t)g].reserve(bytes_per_shard) != ORR_OK || c->xrecv[(size_t)g].reserve(bytes_per_shard * (size_t)G) != ORR_OK)
            return give_up("no device memory for the exchange buffers", nullptr);
    }
    if (c->xhost.reserve(bytes_per_shard * (size_t)G) != ORR_OK) return give_up("no pinned memory for the gathered records", nullptr);
    return ORR_OK;
}

// One all-gather of the shards' records (grouped: one thread drives every device), then device 0's gathered copy -> out.
int rccl_all_gather(orr_cluster *c, size_t bytes_per_shard, orr_candidate *out)
{
    const int G = (int)c->shards.size();
    RcclApi *api = RcclApi::get();
    int r = api->GroupStart();
    for (int g = 0; g < G && r == 0; ++g)
        r = api->AllGather(c->xsend[(size_t)g].p, c->xrecv[(size_t)g].p, bytes_per_shard, /* ncclInt8 */ 0, c->comms[(size_t)g], c->xstreams[(size_t)g]);
    const int r2 = api->GroupEnd();
    if (r == 0) r = r2;
    if (r != 0) { c->exchange = 0; return fail(ORR_ECOMM, "orr_cluster: ncclAllGather failed: %s", api->text(r)); }
    HIP_TRY(hipSetDevice(c->shards[0]->device));
    HIP_TRY(hipMemcpyAsync(c->xhost.p, c->xrecv[0].p, bytes_per_shard * (size_t)G, hipMemcpyDeviceToHost, c->xstreams[0]));
    for (int g = 0; g < G; ++g) {                       // every device's part of the collective is over before the buffers are reused
        HIP_TRY(hipSetDevice(c->shards[(size_t)g]->device));
        HIP_TRY(hipStreamSynchronize(c->xstreams[(size_t)g]));
    }
    memcpy(out, c->xhost.p, bytes_per_shard * (size_t)G);
    c->rccl_exchanges += 1;
    return ORR_OK;
}

// escalate() on a cluster: every pass runs on all shards at once, each shard's half on a lane of that shard that is taken and
// given back inside the pass (concurrent cluster searches take different lanes).  The sub-batch is host memory (the cluster's
// queries are host-resident by contract), built once for all shards.
Backend cluster_backend(orr_cluster *c, int64_t candidate_limit)
{
    const int32_t G = (int32_t)c->shards.size();
    Backend be{"orr_cluster_search_batch", c->dim, c->shards[0], 0, 1, true, &c->sstats, &c->stats_mu, nullptr, nullptr};
    std::vector<int64_t> n_shard;
    for (orr_index *sh : c->shards) {
        n_shard.push_back(participating_rows(sh, candidate_limit));
        be.n_total += n_shard.back();
        be.slice_rows = std::max(be.slice_rows, n_shard.back());
    }
    be.run_pass = [c, G, n_shard](const BatchArgs &cur, int32_t kprime, PassResult &pr) -> int {
        const bool use_cos = cur.dim > 0 && cur.dim == c->dim;
        BatchArgs mine = cur;
        if (use_cos) {
            pr.norm_store.resize((size_t)cur.B);
            exact_norms(cur.q, cur.B, cur.dim, pr.norm_store.data());
            mine.norms_host = pr.norms = pr.norm_store.data();
        }
        pr.q_host = cur.q;
        const size_t rec_per_shard = (size_t)cur.B * ((size_t)kprime + 1);
        pr.rec_store.resize((size_t)G * rec_per_shard);
        pr.recs = pr.rec_store.data();
        pr.shards.resize((size_t)G);
        // "exchange" = 1: the shards write their records into per-device send buffers and ONE RCCL all-gather brings every shard's
        // records to every device; the merge reads device 0's copy.  (One exchange at a time per cluster: the communicators are
        // not shared between concurrent collectives.)
        std::unique_lock<std::mutex> rccl_lock(c->rccl_mu, std::defer_lock);
        bool via_rccl = false;
        const size_t rec_bytes_shard = sizeof(orr_candidate) * rec_per_shard;
        if (c->exchange == 1) {
            rccl_lock.lock();
            via_rccl = rccl_prepare(c, rec_bytes_shard) == ORR_OK;
            if (!via_rccl) rccl_lock.unlock();
        }
        // all lanes before any shard starts, here and in ascending shard order (acquire_in_order says why)
        std::vector<Lane> lanes;
        std::vector<LanePool *> pools;
        std::vector<LanePool::Make> makes;
        for (orr_index *sh : c->shards) { pools.push_back(&sh->lanes); makes.push_back(lane_maker(sh)); }
        acquire_in_order(pools, makes, lanes);
        for (int32_t g = 0; g < G; ++g) adopt_survivor_hint(c->shards[(size_t)g], lanes[(size_t)g].lane);
        ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
            orr_index *sh = lanes[(size_t)g].lane;
            std::lock_guard<std::mutex> lock(sh->mu);
            BatchArgs a = mine;
            const float *qh = nullptr;
            const orr_candidate *recs = nullptr;
            orr_candidate *dst = pr.rec_store.data() + (size_t)g * rec_per_shard;
            PassPlan pass;
            if (via_rccl) {
                a.out_dev = c->xsend[(size_t)g].as<orr_candidate>();             // complete when run_shard returns (it synchronises its stream)
                ORR_TRY(run_shard(sh, a, kprime, false, &qh, &recs, pass));
            } else {
                ORR_TRY(run_shard(sh, a, kprime, true, &qh, &recs, pass));
                if (recs) memcpy(dst, recs, rec_bytes_shard);
                else HIP_TRY(hipMemcpy(dst, sh->ws_cand.p, rec_bytes_shard, hipMemcpyDeviceToHost));
            }
            pr.shards[(size_t)g] = outcome_of(sh, pass, n_shard[(size_t)g]);
            return ORR_OK;
        }));
        lanes.clear();
        if (via_rccl) ORR_TRY(rccl_all_gather(c, rec_bytes_shard, pr.rec_store.data()));
        return ORR_OK;
    };
    // a grown size reaches the shard's lanes through their owner: every lane adopts the owner's hint when a search takes it (the
    // repeat may run on another lane than the one that measured the counts)
    be.grow = [c](const std::vector<ShardOutcome> &ran, const std::vector<uint32_t> &new_cap) {
        for (size_t g = 0; g < new_cap.size(); ++g)
            if (new_cap[g] > ran[g].survivor_cap) publish_survivor_hint(c->shards[g], new_cap[g]);
    };
    return be;
}

// ---- scoped and masked search over the shards (orr_cluster_search_batch_scoped, orr_cluster_search_batch_masked) ----------
// The call holds one lane per shard from its first step to its last.  Count: every shard resolves the scope and reports its
// live rows; the host splits the global candidate_limit (cscope::split_limit).  Pass: every shard runs its shard form
// (scoped_shard / masked_shard, which resolve the scope again on the lane: nothing of the count is kept on the device) at k'
// into its slice of one record array in host memory.  Merge: merge_into, as orr_merge_candidates_ex.  Ladder: the uncertified
// queries repeat as a compacted sub-batch on the next rung (cscope::next_rung).  The rules are orr_cluster_scope_plan.h's.
// With a handle (orr_cluster_search_batch_in_scope) there is no count step: the counts are the handles' own, read behind the
// lanes and the shared holds, and the shard form takes each shard's part as it lies (orr_cluster_handle_plan.h).
struct ClusterScope {
    bool masked;                   // one list shared by the batch through the masked shard form; else per-query lists (off) or a shared one
    int64_t n_ids;
    const int64_t *ids;            // host
    const uint64_t *off;           // host [B + 1] or null
    const orr_cluster_scope *handle = nullptr;   // masked, instead of the list (orr_cluster_search_batch_in_scope)
};

// The cluster of a cluster scope, or ORR_ESTATE: orphaned.
int cluster_scope_owner(const orr_cluster_scope *s, const char *fn, orr_cluster **c)
{
    *c = s->owner.load();
    if (!*c) return fail(ORR_ESTATE, "%s: the cluster scope is orphaned: its cluster was destroyed, or an edit of it failed on some shards", fn);
    return ORR_OK;
}

// What every cluster scope call does first: the outputs empty, the call counted.
void cluster_scope_begin(orr_cluster *c, const BatchArgs &orig, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t B = orig.B, take = std::max<int32_t>(1, orig.topk);
    for (size_t i = 0; i < (size_t)B * take; ++i) { out_rows[i] = -1; out_scores[i] = 0.0; }
    if (out_counts) for (int32_t b = 0; b < B; ++b) out_counts[b] = 0;
    std::lock_guard<std::mutex> l(c->stats_mu);
    c->sstats.searches += 1;
    c->sstats.queries += B;
}

// All lanes before any shard starts, in ascending shard order (acquire_in_order says why), kept for the call.
void cluster_scope_lanes(orr_cluster *c, std::vector<Lane> &lanes)
{
    std::vector<LanePool *> pools;
    std::vector<LanePool::Make> makes;
    for (orr_index *sh : c->shards) { pools.push_back(&sh->lanes); makes.push_back(lane_maker(sh)); }
    acquire_in_order(pools, makes, lanes);
    for (size_t g = 0; g < c->shards.size(); ++g) adopt_survivor_hint(c->shards[g], lanes[g].lane);
}

int cluster_scope_on_lanes(orr_cluster *c, const char *fn, const BatchArgs &orig, const ClusterScope &cs, std::vector<Lane> &lanes,
                           bool handle_held, bool requery, int64_t *out_rows, double *out_scores, int32_t *out_counts);

int cluster_scope_search(orr_cluster *c, const char *fn, const BatchArgs &orig, const ClusterScope &cs, int64_t *out_rows, double *out_scores,
                         int32_t *out_counts)
{
    cluster_scope_begin(c, orig, out_rows, out_scores, out_counts);
    if (!cs.handle && cs.n_ids == 0) return ORR_OK;
    std::vector<Lane> lanes;
    cluster_scope_lanes(c, lanes);
    return cluster_scope_on_lanes(c, fn, orig, cs, lanes, false, false, out_rows, out_scores, out_counts);
}

// The search on the lanes the caller took.  handle_held: the caller holds the handle's parts shared already (a grouped call,
// which holds several); requery: the queries come from a pass that left them uncertified, and count as requeried from the
// first rung on.  The outputs are the caller's, emptied.
int cluster_scope_on_lanes(orr_cluster *c, const char *fn, const BatchArgs &orig, const ClusterScope &cs, std::vector<Lane> &lanes,
                           bool handle_held, bool requery, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t G = (int32_t)c->shards.size(), B = orig.B, take = std::max<int32_t>(1, orig.topk);
    const bool use_cos = orig.dim > 0 && orig.dim == c->dim;
    std::vector<double> norms;
    if (use_cos) {
        norms.resize((size_t)B);
        exact_norms(orig.q, B, orig.dim, norms.data());
    }

    // ---- count: live[g][b] (masked: one number per shard), then the split
    const bool shared = cs.off == nullptr;
    const int32_t nq = shared ? 1 : B;
    std::vector<int64_t> live((size_t)G * (size_t)nq, 0);
    const ScopeArgs whole{cs.n_ids, cs.ids, cs.off, nullptr};
    std::vector<cscope::Split> split((size_t)nq);          // per query (a shared list: one for all)
    // a handle: no count step.  Behind the lanes (no delete, compaction or insertion runs on a shard whose lane is held) every
    // shard's scope is taken shared in ascending shard order, and the counts are the handles' own.
    std::vector<std::shared_lock<std::shared_mutex>> held;
    if (cs.handle) {
        held.reserve((size_t)G);
        for (int32_t g = 0; g < G && !handle_held; ++g) held.emplace_back(cs.handle->parts[(size_t)g]->mu);
        for (int32_t g = 0; g < G; ++g) {
            const orr_scope *part = cs.handle->parts[(size_t)g];
            orr_index *own = nullptr;
            ORR_TRY(scope_owner(part, c->shards[(size_t)g], fn, &own));
            if (part->n_rows != lanes[(size_t)g].lane->n_rows)
                return fail(ORR_ESTATE, "%s: the scope covers %lld rows of shard %d, the shard holds %lld", fn, (long long)part->n_rows, g, (long long)lanes[(size_t)g].lane->n_rows);
            live[(size_t)g] = part->live.load();
        }
        if (!chandle::handle_split(live, orig.candidate_limit, split[0])) return fail(ORR_ESTATE, "%s: a shard's scope is orphaned", fn);
    } else {
        ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
            orr_index *sh = lanes[(size_t)g].lane;
            std::lock_guard<std::mutex> lock(sh->mu);
            return scope_count_on_lane(sh, nq, whole, live.data() + (size_t)g * (size_t)nq);
        }));
        for (int32_t b = 0; b < nq; ++b) {
            std::vector<int64_t> col((size_t)G);
            for (int32_t g = 0; g < G; ++g) col[(size_t)g] = live[(size_t)g * (size_t)nq + (size_t)b];
            split[(size_t)b] = cscope::split_limit(col, orig.candidate_limit);
        }
    }
    auto split_of = [&](int32_t b) -> const cscope::Split & { return split[shared ? 0 : (size_t)b]; };

    // ---- the ladder
    struct Todo { std::vector<int32_t> ids; cscope::Rung rung; int repeats; };
    Todo first{{}, {}, 0};
    int64_t total = 0;
    for (int32_t b = 0; b < B; ++b)
        if (split_of(b).total > 0) { first.ids.push_back(b); total = std::max(total, split_of(b).total); }
    if (first.ids.empty()) return ORR_OK;
    first.rung = cscope::first_rung(cs.masked, take, total, orr::kSelWidth);
    std::deque<Todo> todo(1, std::move(first));
    while (!todo.empty()) {
        const Todo r = std::move(todo.front());
        todo.pop_front();
        const int32_t n_ids = (int32_t)r.ids.size(), kprime = (int32_t)std::min<int64_t>(r.rung.kprime, std::numeric_limits<int32_t>::max() - 1);
        const size_t rec_q = (size_t)kprime + 1;
        const int32_t per = cscope::merge_slice(n_ids, G, kprime, mask::kMergeBudgetBytes);
        Todo next{{}, {}, r.repeats + 1};
        int64_t largest = 0;
        bool screened = false;
        for (int32_t i0 = 0; i0 < n_ids; i0 += per) {
            const std::vector<int32_t> ids(r.ids.begin() + i0, r.ids.begin() + std::min<int32_t>(n_ids, i0 + per));
            const int32_t nb = (int32_t)ids.size();
            SubBatch sb;
            BatchArgs cur;
            ORR_TRY(build_subset(lanes[0].lane, orig, ids, sb, cur));                  // (host-resident vectors: nothing of the lane is used)
            std::vector<double> sub_norms((size_t)nb, 0.0);
            if (use_cos) for (int32_t i = 0; i < nb; ++i) sub_norms[(size_t)i] = norms[(size_t)ids[(size_t)i]];
            // the scopes of the sub-batch: a shared list as it is, per-query lists gathered in the sub-batch's order
            std::vector<int64_t> sub_ids;
            std::vector<uint64_t> sub_off;
            ScopeArgs sc{cs.n_ids, cs.ids, cs.off, nullptr};
            if (!shared && cur.B != orig.B) {
                sub_off.assign(1, 0);
                for (int32_t b : ids) {
                    sub_ids.insert(sub_ids.end(), cs.ids + cs.off[b], cs.ids + cs.off[b + 1]);
                    sub_off.push_back((uint64_t)sub_ids.size());
                }
                if (sub_ids.empty()) sub_ids.push_back(-1);                            // (every list empty: an id no row carries)
                sc = ScopeArgs{(int64_t)sub_off.back(), sub_ids.data(), sub_off.data(), nullptr};
            }
            std::vector<int64_t> before((size_t)G * (size_t)nb);
            for (int32_t g = 0; g < G; ++g)
                for (int32_t i = 0; i < nb; ++i) before[(size_t)g * (size_t)nb + (size_t)i] = split_of(ids[(size_t)i]).before[(size_t)g];
            std::vector<orr_candidate> recs((size_t)G * (size_t)nb * rec_q);
            ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
                orr_index *sh = lanes[(size_t)g].lane;
                std::lock_guard<std::mutex> lock(sh->mu);
                BatchArgs a = cur;
                a.topk = std::min<int32_t>(kprime, take);                              // the floor's k: the global k-th best is at least every shard's
                if (use_cos) a.norms_host = sub_norms.data();
                orr_candidate *dst = recs.data() + (size_t)g * (size_t)nb * rec_q;
                sh->sstats.searches += 1; sh->sstats.queries += nb;
                if (cs.handle) return masked_shard(sh, a, ScopeSource{nullptr, cs.handle->parts[(size_t)g]}, before[(size_t)g * (size_t)nb], kprime, r.rung.pass, dst);
                if (cs.masked) return masked_shard(sh, a, ScopeSource{&sc, nullptr}, before[(size_t)g * (size_t)nb], kprime, r.rung.pass, dst);
                ScopeArgs mine = sc;
                mine.before = before.data() + (size_t)g * (size_t)nb;
                return scoped_shard(sh, a, mine, kprime, dst);
            }));
            std::vector<uint8_t> cert;
            ORR_TRY(merge_into(G, kprime, recs.data(), cur, use_cos, cur.q, use_cos ? sub_norms.data() : nullptr, ids, out_rows, out_scores, out_counts, cert));
            for (int32_t i = 0; i < nb; ++i) {
                if (cert[(size_t)i]) continue;
                next.ids.push_back(ids[(size_t)i]);
                largest = std::max(largest, split_of(ids[(size_t)i]).largest);
                for (int32_t g = 0; g < G; ++g)
                    screened = screened || (recs[((size_t)g * (size_t)nb + (size_t)i) * rec_q + (size_t)kprime].flags & ORR_CAND_TWO_STAGE) != 0;
            }
            std::lock_guard<std::mutex> l(c->stats_mu);
            c->sstats.passes += 1;
            c->sstats.pass_mode = cs.masked && r.rung.pass == 0 ? 5 : 4;
            if (r.repeats > 0 || requery) c->sstats.requeried += nb;
        }
        if (next.ids.empty()) continue;
        next.rung = cscope::next_rung(r.rung, cs.masked, screened, largest, orr::kSelWidth);
        if (next.rung.done || next.repeats >= cscope::kMaxRungs)
            return fail(ORR_EDEVICE, "%s: a pass with every scoped row a record left a query uncertified", fn);
        todo.push_front(std::move(next));
    }
    return ORR_OK;
}

// ---- grouped search over the shards (orr_cluster_search_batch_in_scopes; the rules are orr_cluster_group_plan.h's) -----------
// The queries `ids` of the call (ascending, all of one handle) through the in-scope cluster ladder of that handle, on the lanes
// and holds the caller took, the results scattered back.
int cluster_scope_sub(orr_cluster *c, const char *fn, const BatchArgs &orig, const orr_cluster_scope *handle, const std::vector<int32_t> &ids,
                      std::vector<Lane> &lanes, bool requery, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    if (ids.empty()) return ORR_OK;
    const int32_t take = std::max<int32_t>(1, orig.topk);
    ClusterScope cs{true, 0, nullptr, nullptr};
    cs.handle = handle;
    SubBatch sb;
    BatchArgs cur;
    ORR_TRY(build_subset(lanes[0].lane, orig, ids, sb, cur));          // (host-resident vectors: nothing of the lane is used)
    if (cur.B == orig.B) return cluster_scope_on_lanes(c, fn, cur, cs, lanes, true, requery, out_rows, out_scores, out_counts);
    const size_t nb = ids.size();
    std::vector<int64_t> rows(nb * (size_t)take, -1);
    std::vector<double> scores(nb * (size_t)take, 0.0);
    std::vector<int32_t> counts(nb, 0);
    std::vector<int64_t> keys(orig.out_keys ? nb * (size_t)take : 0, -1);      // (out_keys is in the numbering of the call that receives it)
    if (orig.out_keys) cur.out_keys = keys.data();
    ORR_TRY(cluster_scope_on_lanes(c, fn, cur, cs, lanes, true, requery, rows.data(), scores.data(), counts.data()));
    for (size_t i = 0; i < nb; ++i) {
        const size_t b = (size_t)ids[i];
        if (orig.out_keys) memcpy(orig.out_keys + b * take, keys.data() + i * take, sizeof(int64_t) * take);
        memcpy(out_rows + b * take, rows.data() + i * take, sizeof(int64_t) * take);
        memcpy(out_scores + b * take, scores.data() + i * take, sizeof(double) * take);
        if (out_counts) out_counts[b] = counts[i];
    }
    return ORR_OK;
}

int cluster_grouped_on_lanes(orr_cluster *c, const char *fn, const BatchArgs &orig, int32_t n_scopes, const orr_cluster_scope *const *scopes,
                             const int32_t *query_scope, std::vector<Lane> &lanes, int64_t *out_rows, double *out_scores, int32_t *out_counts);

int cluster_grouped_search(orr_cluster *c, const char *fn, const BatchArgs &orig, int32_t n_scopes, const orr_cluster_scope *const *scopes,
                           const int32_t *query_scope, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    cluster_scope_begin(c, orig, out_rows, out_scores, out_counts);
    std::vector<Lane> lanes;
    cluster_scope_lanes(c, lanes);
    return cluster_grouped_on_lanes(c, fn, orig, n_scopes, scopes, query_scope, lanes, out_rows, out_scores, out_counts);
}

// The grouped search on the lanes the caller took (orr_cluster_search_batch_per_key runs its later rounds through it on the one
// set of lanes it holds).  The outputs are the caller's, emptied; orig.out_keys, if set, receives each result's order_key.
int cluster_grouped_on_lanes(orr_cluster *c, const char *fn, const BatchArgs &orig, int32_t n_scopes, const orr_cluster_scope *const *scopes,
                             const int32_t *query_scope, std::vector<Lane> &lanes, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t G = (int32_t)c->shards.size(), B = orig.B, take = std::max<int32_t>(1, orig.topk);
    const bool use_cos = orig.dim > 0 && orig.dim == c->dim;
    // ---- the groups: the distinct handles; their parts shared, in one total order, behind the lanes
    std::vector<uintptr_t> addr((size_t)n_scopes);
    for (int32_t i = 0; i < n_scopes; ++i) addr[(size_t)i] = reinterpret_cast<uintptr_t>(scopes[i]);
    const cgroup::Distinct dis = cgroup::distinct(addr);
    const int32_t D = (int32_t)dis.first.size();
    std::vector<const orr_cluster_scope *> handle((size_t)D);
    std::vector<std::vector<uintptr_t>> parts((size_t)D, std::vector<uintptr_t>((size_t)G));
    for (int32_t d = 0; d < D; ++d) {
        handle[(size_t)d] = scopes[dis.first[(size_t)d]];
        for (int32_t g = 0; g < G; ++g) parts[(size_t)d][(size_t)g] = reinterpret_cast<uintptr_t>(handle[(size_t)d]->parts[(size_t)g]);
    }
    std::vector<std::shared_lock<std::shared_mutex>> held;
    const std::vector<cgroup::Hold> order = cgroup::holds(parts);
    held.reserve(order.size());
    for (const cgroup::Hold &h : order) held.emplace_back(handle[(size_t)h.group]->parts[(size_t)h.shard]->mu);
    std::vector<std::vector<int64_t>> live((size_t)D, std::vector<int64_t>((size_t)G, 0));
    for (int32_t d = 0; d < D; ++d)
        for (int32_t g = 0; g < G; ++g) {
            const orr_scope *part = handle[(size_t)d]->parts[(size_t)g];
            orr_index *own = nullptr;
            ORR_TRY(scope_owner(part, c->shards[(size_t)g], fn, &own));
            if (part->n_rows != lanes[(size_t)g].lane->n_rows)
                return fail(ORR_ESTATE, "%s: a scope covers %lld rows of shard %d, the shard holds %lld", fn, (long long)part->n_rows, g, (long long)lanes[(size_t)g].lane->n_rows);
            live[(size_t)d][(size_t)g] = part->live.load();
        }
    std::vector<cscope::Split> split;
    if (!cgroup::splits(live, orig.candidate_limit, split)) return fail(ORR_ESTATE, "%s: a shard's scope is orphaned", fn);
    std::vector<int32_t> qgroup((size_t)B);
    for (int32_t b = 0; b < B; ++b) qgroup[(size_t)b] = dis.group_of[(size_t)query_scope[b]];
    const cgroup::First first = cgroup::first(split, qgroup);
    if (first.n_used == 0) return ORR_OK;
    // one used group: the in-scope cluster call itself, nothing new runs
    if (first.n_used == 1) return cluster_scope_sub(c, fn, orig, handle[(size_t)first.only], first.ids, lanes, false, out_rows, out_scores, out_counts);

    // ---- the first rung: every shard runs its grouped shard form once
    std::vector<double> norms;
    if (use_cos) {
        norms.resize((size_t)B);
        exact_norms(orig.q, B, orig.dim, norms.data());
    }
    const cscope::Rung rung = cscope::first_rung(true, take, first.total, orr::kSelWidth);
    const int32_t n_ids = (int32_t)first.ids.size(), kprime = (int32_t)std::min<int64_t>(rung.kprime, std::numeric_limits<int32_t>::max() - 1);
    const size_t rec_q = (size_t)kprime + 1;
    const int32_t per = cscope::merge_slice(n_ids, G, kprime, mask::kMergeBudgetBytes);
    std::vector<std::vector<int32_t>> again((size_t)D);
    bool any_grouped = false;
    for (int32_t i0 = 0; i0 < n_ids; i0 += per) {
        const std::vector<int32_t> ids(first.ids.begin() + i0, first.ids.begin() + std::min<int32_t>(n_ids, i0 + per));
        const int32_t nb = (int32_t)ids.size();
        SubBatch sb;
        BatchArgs cur;
        ORR_TRY(build_subset(lanes[0].lane, orig, ids, sb, cur));                      // (host-resident vectors: nothing of the lane is used)
        std::vector<double> sub_norms((size_t)nb, 0.0);
        std::vector<int32_t> sub_group((size_t)nb);
        for (int32_t i = 0; i < nb; ++i) {
            if (use_cos) sub_norms[(size_t)i] = norms[(size_t)ids[(size_t)i]];
            sub_group[(size_t)i] = qgroup[(size_t)ids[(size_t)i]];
        }
        std::vector<orr_candidate> recs((size_t)G * (size_t)nb * rec_q);
        std::vector<uint8_t> ran((size_t)G, 0);
        ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
            orr_index *sh = lanes[(size_t)g].lane;
            std::lock_guard<std::mutex> lock(sh->mu);
            BatchArgs a = cur;
            a.topk = std::min<int32_t>(kprime, take);                                  // the floor's k: the global k-th best is at least every shard's
            if (use_cos) a.norms_host = sub_norms.data();
            std::vector<const orr_scope *> mine((size_t)D);
            std::vector<int64_t> before((size_t)D);
            for (int32_t d = 0; d < D; ++d) { mine[(size_t)d] = handle[(size_t)d]->parts[(size_t)g]; before[(size_t)d] = split[(size_t)d].before[(size_t)g]; }
            GroupArgs ga{D, 0, nullptr, nullptr, sub_group.data()};
            ga.scopes = mine.data();
            sh->sstats.searches += 1; sh->sstats.queries += nb;
            bool grouped = false;
            const int rc = grouped_shard(sh, a, ga, before.data(), kprime, rung.pass, recs.data() + (size_t)g * (size_t)nb * rec_q, &grouped);
            ran[(size_t)g] = grouped ? 1 : 0;
            return rc;
        }));
        std::vector<uint8_t> cert;
        ORR_TRY(merge_into(G, kprime, recs.data(), cur, use_cos, cur.q, use_cos ? sub_norms.data() : nullptr, ids, out_rows, out_scores, out_counts, cert));
        cgroup::route(ids, cert, qgroup, again);
        bool grouped = false;
        for (int32_t g = 0; g < G; ++g) grouped = grouped || ran[(size_t)g] != 0;
        any_grouped = any_grouped || grouped;
        std::lock_guard<std::mutex> l(c->stats_mu);
        c->sstats.passes += 1;
        c->sstats.pass_mode = grouped ? 6 : rung.pass == 0 ? 5 : 4;
    }
    // ---- every uncertified query: its own group's ladder, with the group's others
    for (int32_t d = 0; d < D; ++d) {
        if (again[(size_t)d].empty()) continue;
        for (int32_t b : again[(size_t)d]) {           // (the ladder's merge writes every slot of a query it certifies; start from empty)
            for (int32_t t = 0; t < take; ++t) { out_rows[(size_t)b * take + t] = -1; out_scores[(size_t)b * take + t] = 0.0; }
            if (out_counts) out_counts[b] = 0;
        }
        ORR_TRY(cluster_scope_sub(c, fn, orig, handle[(size_t)d], again[(size_t)d], lanes, true, out_rows, out_scores, out_counts));
    }
    if (any_grouped) {                                 // (pass_mode tells that a grouped pass ran, whatever a group's own ladder ran after it)
        std::lock_guard<std::mutex> l(c->stats_mu);
        c->sstats.pass_mode = 6;
    }
    return ORR_OK;
}

// The checks the two calls share; the cluster's shared lock is the caller's.
int check_cluster_scope(orr_cluster *c, const char *fn, const BatchArgs &a, const ClusterScope &cs, const int64_t *out_rows, const double *out_scores)
{
    ORR_TRY(check_scope_args(a.B, ScopeArgs{cs.n_ids, cs.ids, cs.off, nullptr}, fn));       // (the scope before the handle, as the index calls check)
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (a.B <= 0) return fail(ORR_EINVAL, "%s: batch size must be positive", fn);
    if (a.dim < 0) return fail(ORR_EINVAL, "%s: negative query dimension", fn);
    if (a.dim > 0 && !a.q) return fail(ORR_EINVAL, "%s: q is NULL with dim %d", fn, a.dim);
    if (!a.query_term_off) return fail(ORR_EINVAL, "%s: query_term_off is required", fn);
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "%s: output buffers are required", fn);
    if (a.dim > 0 && is_device_pointer(a.q)) return fail(ORR_EINVAL, "%s: the query vectors must be in host memory (every shard's device reads them)", fn);
    if (cs.n_ids > 0 && is_device_pointer(cs.ids)) return fail(ORR_EINVAL, "%s: scope_ids must be in host memory (every shard's device reads them)", fn);
    return ORR_OK;
}

int cluster_scope_call(orr_cluster *c, const char *fn, const BatchArgs &a, const ClusterScope &cs, int64_t *out_rows, double *out_scores,
                       int32_t *out_counts)
{
    ORR_TRY(check_cluster_scope(c, fn, a, cs, out_rows, out_scores));
    std::shared_lock<std::shared_mutex> lock(c->mu);   // searches run side by side; seal and destroy are exclusive
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    return cluster_scope_search(c, fn, a, cs, out_rows, out_scores, out_counts);
}

}  // namespace

static int cluster_plain_search(orr_cluster *c, const BatchArgs &a, int64_t *out_rows, double *out_scores, int32_t *out_counts);

extern "C" {

int orr_cluster_create(const int32_t *devices, int32_t n_shards, int32_t dim, int64_t capacity_rows_per_shard, orr_cluster **out)
{
    if (!devices || !out || n_shards < 1 || n_shards > 64 || dim < 0 || capacity_rows_per_shard < 0)
        return fail(ORR_EINVAL, "orr_cluster_create: bad argument");
    *out = nullptr;
    orr_cluster *c = new (std::nothrow) orr_cluster();
    if (!c) return fail(ORR_ENOMEM, "out of host memory");
    c->dim = dim;
    for (int32_t i = 0; i < n_shards; ++i) {
        orr_config cfg{(int32_t)sizeof(orr_config), devices[i], dim, 0, capacity_rows_per_shard, 0};
        orr_index *sh = nullptr;
        const int r = orr_index_create(&cfg, &sh);
        if (r != ORR_OK) { const std::string keep = g_last_error; orr_cluster_destroy(c); g_last_error = keep; return r; }
        c->shards.push_back(sh);
    }
    *out = c;
    return ORR_OK;
}

void orr_cluster_destroy(orr_cluster *c)
{
    if (!c) return;
    if (!c->comms.empty()) {
        RcclApi *api = RcclApi::get();
        for (size_t g = 0; g < c->comms.size(); ++g) {
            if (g < c->shards.size()) (void)hipSetDevice(c->shards[g]->device);
            if (g < c->xstreams.size() && c->xstreams[g]) { (void)hipStreamSynchronize(c->xstreams[g]); (void)hipStreamDestroy(c->xstreams[g]); }
            if (c->comms[g] && api->CommDestroy) (void)api->CommDestroy(c->comms[g]);
            if (g < c->xsend.size()) c->xsend[g].release();
            if (g < c->xrecv.size()) c->xrecv[g].release();
        }
    }
    c->xhost.release();
    {   // cluster scopes that are still alive are orphaned before their shards go (each shard then orphans its part)
        std::lock_guard<std::mutex> life(g_scope_life_mu);
        for (orr_cluster_scope *s : c->cscopes) s->owner.store(nullptr);
        c->cscopes.clear();
        for (orr_cluster_keys *k : c->ckeys) k->owner.store(nullptr);
        c->ckeys.clear();
    }
    for (orr_index *sh : c->shards) orr_index_destroy(sh);
    delete c;
}

int orr_cluster_set_option(orr_cluster *c, const char *name, int64_t value)
{
    if (!c || !name) return fail(ORR_EINVAL, "orr_cluster_set_option: null argument");
    std::unique_lock<std::shared_mutex> lock(c->mu);
    if (strcmp(name, "exchange") == 0) {
        if (value != 0 && value != 1) return fail(ORR_EINVAL, "orr_cluster_set_option: exchange takes 0 (pinned host memory) or 1 (RCCL all-gather)");
        if (value == 1) {
            if (!RcclApi::get()->ok()) return fail(ORR_ECOMM, "orr_cluster_set_option: librccl.so could not be loaded");
            for (size_t g = 0; g < c->shards.size(); ++g)
                for (size_t h = 0; h < g; ++h)
                    if (c->shards[h]->device == c->shards[g]->device)
                        return fail(ORR_EINVAL, "orr_cluster_set_option: the RCCL exchange needs every shard on a device of its own (shards %zu and %zu share device %d)",
                                    h, g, c->shards[g]->device);
        }
        std::lock_guard<std::mutex> l(c->rccl_mu);
        c->exchange = (int)value;
        return ORR_OK;
    }
    return fail(ORR_EINVAL, "orr_cluster_set_option: unknown option %s", name);
}

int32_t orr_cluster_shards(const orr_cluster *c) { return c ? (int32_t)c->shards.size() : 0; }

orr_index *orr_cluster_shard(orr_cluster *c, int32_t i)
{
    if (!c || i < 0 || i >= (int32_t)c->shards.size()) { (void)fail(ORR_EINVAL, "orr_cluster_shard: no shard %d", i); return nullptr; }
    return c->shards[(size_t)i];
}

int64_t orr_cluster_rows(const orr_cluster *c)
{
    int64_t n = 0;
    if (c) for (const orr_index *sh : c->shards) n += sh->n_rows;
    return n;
}

int orr_cluster_seal(orr_cluster *c)
{
    if (!c) return fail(ORR_EINVAL, "orr_cluster_seal: null cluster");
    std::unique_lock<std::shared_mutex> lock(c->mu);
    ORR_TRY(for_each_shard((int32_t)c->shards.size(), [&](int32_t g) { return orr_index_seal(c->shards[(size_t)g]); }));
    int64_t base = 0, dead = 0;
    const orr_index *prev = nullptr;
    for (orr_index *sh : c->shards) {
        // the global candidate order must be shard 0's rows, then shard 1's, ...: nothing in a shard may be newer than a row in front of it
        if (prev && !prev->h_created.empty() && !sh->h_created.empty() && sh->h_created.front() > prev->h_created.back())
            return fail(ORR_EINVAL, "orr_cluster_seal: a shard holds a row newer than one of the shard in front of it; "
                                    "partition the rows by CreatedAtUtc, newest first");
        ORR_TRY(orr_index_set_row_base(sh, base));
        ORR_TRY(orr_index_set_option(sh, "dead_rows_before", dead));
        base += sh->n_rows;
        dead += (int64_t)sh->dead.size();
        if (sh->n_rows > 0) prev = sh;
    }
    c->sealed = true;
    return ORR_OK;
}

// places the shards in the global candidate order: row_base and the deleted rows in front of each
static int place_shards(orr_cluster *c)
{
    int64_t base = 0, dead = 0;
    for (orr_index *sh : c->shards) {
        ORR_TRY(orr_index_set_row_base(sh, base));
        ORR_TRY(orr_index_set_option(sh, "dead_rows_before", dead));
        base += sh->n_rows;
        dead += (int64_t)sh->dead.size();
    }
    return ORR_OK;
}

int orr_cluster_compact(orr_cluster *c, int64_t *out_removed)
{
    if (out_removed) *out_removed = 0;
    if (!c) return fail(ORR_EINVAL, "orr_cluster_compact: null cluster");
    std::unique_lock<std::shared_mutex> lock(c->mu);   // no search in flight on the cluster
    if (!c->sealed) return fail(ORR_ESTATE, "orr_cluster_compact: the cluster is not sealed");
    std::vector<int64_t> removed(c->shards.size(), 0);
    ORR_TRY(for_each_shard((int32_t)c->shards.size(), [&](int32_t g) { return orr_index_compact(c->shards[(size_t)g], &removed[(size_t)g]); }));
    ORR_TRY(place_shards(c));                          // the shards behind a compacted one move up in the global order
    if (out_removed) for (int64_t r : removed) *out_removed += r;
    return ORR_OK;
}

int orr_cluster_insert_rows(orr_cluster *c, int32_t shard, int64_t n, int32_t dim, const float *emb, const int64_t *created_ticks,
                            const uint8_t *content_lower, const uint64_t *content_off, const int64_t *row_ids, int64_t *out_inserted)
{
    if (out_inserted) *out_inserted = 0;
    if (!c) return fail(ORR_EINVAL, "orr_cluster_insert_rows: null cluster");
    if (shard < 0 || shard >= (int32_t)c->shards.size()) return fail(ORR_EINVAL, "orr_cluster_insert_rows: no shard %d", shard);
    if (n < 0) return fail(ORR_EINVAL, "orr_cluster_insert_rows: negative row count");
    if (n > 0 && !created_ticks) return fail(ORR_EINVAL, "orr_cluster_insert_rows: created_ticks are required");
    std::unique_lock<std::shared_mutex> lock(c->mu);   // no search in flight on the cluster
    if (!c->sealed) return fail(ORR_ESTATE, "orr_cluster_insert_rows: the cluster is not sealed");
    if (n > 0) {
        // the order orr_cluster_seal checks, BEFORE anything is written: the new rows against the nearest non-empty neighbours
        orr_index *sh = c->shards[(size_t)shard];
        ORR_TRY(bind_device(sh));
        std::vector<int64_t> ticks((size_t)n);
        HIP_TRY(hipMemcpy(ticks.data(), created_ticks, sizeof(int64_t) * (size_t)n, hipMemcpyDefault));
        const auto mm = std::minmax_element(ticks.begin(), ticks.end());
        for (int32_t g = shard - 1; g >= 0; --g)
            if (!c->shards[(size_t)g]->h_created.empty()) {
                if (*mm.second > c->shards[(size_t)g]->h_created.back())
                    return fail(ORR_EINVAL, "orr_cluster_insert_rows: a row is newer than a row of shard %d in front of shard %d", g, shard);
                break;
            }
        for (int32_t g = shard + 1; g < (int32_t)c->shards.size(); ++g)
            if (!c->shards[(size_t)g]->h_created.empty()) {
                if (*mm.first < c->shards[(size_t)g]->h_created.front())
                    return fail(ORR_EINVAL, "orr_cluster_insert_rows: a row is older than a row of shard %d behind shard %d", g, shard);
                break;
            }
    }
    ORR_TRY(orr_index_insert_rows(c->shards[(size_t)shard], n, dim, emb, created_ticks, content_lower, content_off, row_ids, out_inserted));
    return place_shards(c);                            // the shards behind it move down in the global order
}

int orr_cluster_search_batch(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const uint8_t *terms_utf8,
                             const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                             int64_t candidate_limit, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    if (!c) return fail(ORR_EINVAL, "orr_cluster_search_batch: null cluster");
    BatchArgs a{B, dim, q_host, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    ORR_TRY(check_batch(c->shards[0], a, "orr_cluster_search_batch"));
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "orr_cluster_search_batch: output buffers are required");
    if (dim > 0 && is_device_pointer(q_host)) return fail(ORR_EINVAL, "orr_cluster_search_batch: the query vectors must be in host memory (every shard's device reads them)");
    std::shared_lock<std::shared_mutex> lock(c->mu);   // searches run side by side; seal and destroy are exclusive
    if (!c->sealed) return fail(ORR_ESTATE, "orr_cluster_search_batch: the cluster is not sealed");
    return cluster_plain_search(c, a, out_rows, out_scores, out_counts);
}

}  // extern "C"

// orr_cluster_search_batch behind its checks, the cluster held shared (orr_cluster_search_batch_diverse runs its pool through it)
static int cluster_plain_search(orr_cluster *c, const BatchArgs &a, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const int32_t B = a.B, topk = a.topk;
    const int64_t candidate_limit = a.candidate_limit;
    {   // rows deleted from a shard since the seal (orr_index_delete_rows on orr_cluster_shard(i)) shift the candidate_limit prefix
        // of every shard behind it: when the dead-row prefix sums changed they are set again (an option of the shard: every lane
        // of it is idle while it changes)
        int64_t dead = 0;
        for (orr_index *sh : c->shards) {
            const LanePool::Shared pub = sh->lanes.shared();
            if (pub.dead_before != dead) ORR_TRY(orr_index_set_option(sh, "dead_rows_before", dead));
            dead += pub.dead_count;
        }
    }
    const int32_t take = std::max<int32_t>(1, topk);
    const Backend be = cluster_backend(c, candidate_limit);
    {
        std::lock_guard<std::mutex> l(c->stats_mu);
        c->sstats.searches += 1;
        c->sstats.queries += B;
    }
    for (int64_t i = 0; i < (int64_t)B * take; ++i) { out_rows[i] = -1; out_scores[i] = 0.0; }
    // k' per shard as orr_search_batch picks it for one shard: any shard may hold the whole top-k
    return escalate(be, a, escalation::initial_kprime(take, be.n_total, orr::kSelWidth), out_rows, out_scores, out_counts);
}

extern "C" {

int orr_cluster_search_batch_scoped(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const uint8_t *terms_utf8,
                                    const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                    int64_t candidate_limit, int64_t n_scope_ids, const int64_t *scope_ids, const uint64_t *scope_off,
                                    int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const BatchArgs a{B, dim, q_host, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    return cluster_scope_call(c, "orr_cluster_search_batch_scoped", a, ClusterScope{false, n_scope_ids, scope_ids, scope_off}, out_rows, out_scores, out_counts);
}

int orr_cluster_search_batch_masked(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const uint8_t *terms_utf8,
                                    const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                    int64_t candidate_limit, int64_t n_scope_ids, const int64_t *scope_ids,
                                    int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    const BatchArgs a{B, dim, q_host, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    return cluster_scope_call(c, "orr_cluster_search_batch_masked", a, ClusterScope{true, n_scope_ids, scope_ids, nullptr}, out_rows, out_scores, out_counts);
}

int orr_cluster_search_stats(orr_cluster *c, orr_search_stats *out, int32_t reset)
{
    if (!c) return fail(ORR_EINVAL, "orr_cluster_search_stats: null cluster");
    std::lock_guard<std::mutex> lock(c->stats_mu);
    if (out) { *out = c->sstats; out->reserved[0] = c->rccl_exchanges; }
    if (reset) c->sstats = orr_search_stats{};
    return ORR_OK;
}

}  // extern "C"

// ---- cluster scope handles (orr_cluster_scope): one orr_scope per shard, the rules are orr_cluster_handle_plan.h's ------------

namespace {

// One lane per shard, in ascending shard order (acquire_in_order says why), for a call that works on every shard.
void acquire_cluster_lanes(orr_cluster *c, std::vector<Lane> &lanes)
{
    std::vector<LanePool *> pools;
    std::vector<LanePool::Make> makes;
    for (orr_index *sh : c->shards) { pools.push_back(&sh->lanes); makes.push_back(lane_maker(sh)); }
    acquire_in_order(pools, makes, lanes);
}

// Every part belongs to its shard of `c` still (none was orphaned on its own); the caller holds the parts.
int cluster_scope_parts_alive(const orr_cluster *c, const orr_cluster_scope *s, const char *fn)
{
    for (size_t g = 0; g < s->parts.size(); ++g) {
        orr_index *own = nullptr;
        ORR_TRY(scope_owner(s->parts[g], c->shards[g], fn, &own));
    }
    return ORR_OK;
}

// The cluster scope can no longer be used (ORR_ESTATE from now on); its parts stay with their shards until it is destroyed.
void orphan_cluster_scope(orr_cluster_scope *s)
{
    std::lock_guard<std::mutex> life(g_scope_life_mu);
    orr_cluster *c = s->owner.load();
    if (!c) return;
    c->cscopes.erase(std::remove(c->cscopes.begin(), c->cscopes.end(), s), c->cscopes.end());
    s->owner.store(nullptr);
}

// A new cluster scope: make(shard, &part) on every shard at once.  A failure on any shard destroys the parts already made.
int make_cluster_scope(orr_cluster *c, const char *fn, orr_cluster_scope **out, const std::function<int(orr_index *, orr_scope **)> &make)
{
    std::shared_lock<std::shared_mutex> lock(c->mu);   // like a search: beside the others; seal, compact, insert are exclusive
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    const int32_t G = (int32_t)c->shards.size();
    orr_cluster_scope *s = new (std::nothrow) orr_cluster_scope();
    if (!s) return fail(ORR_ENOMEM, "out of host memory");
    s->parts.assign((size_t)G, nullptr);
    const int r = for_each_shard(G, [&](int32_t g) -> int { return make(c->shards[(size_t)g], &s->parts[(size_t)g]); });
    if (r != ORR_OK) {
        const std::string keep = g_last_error;
        for (orr_scope *part : s->parts) orr_scope_destroy(part);
        delete s;
        g_last_error = keep;
        return r;
    }
    s->owner.store(c);
    { std::lock_guard<std::mutex> life(g_scope_life_mu); c->cscopes.push_back(s); }
    *out = s;
    return ORR_OK;
}

}  // namespace

extern "C" {

int orr_cluster_scope_create(orr_cluster *c, int64_t n_ids, const int64_t *ids, orr_cluster_scope **out)
{
    static const char *fn = "orr_cluster_scope_create";
    if (!out) return fail(ORR_EINVAL, "%s: out is NULL", fn);
    if (n_ids < 0) return fail(ORR_EINVAL, "%s: n_ids is negative", fn);
    if (n_ids > 0 && !ids) return fail(ORR_EINVAL, "%s: ids is NULL with %lld ids", fn, (long long)n_ids);
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (n_ids > 0 && is_device_pointer(ids)) return fail(ORR_EINVAL, "%s: ids must be in host memory (every shard's device reads them)", fn);
    return make_cluster_scope(c, fn, out, [&](orr_index *sh, orr_scope **part) { return orr_scope_create(sh, n_ids, ids, part); });
}

int orr_cluster_scope_create_ticks(orr_cluster *c, int64_t ticks_from, int64_t ticks_to, orr_cluster_scope **out)
{
    static const char *fn = "orr_cluster_scope_create_ticks";
    if (!out) return fail(ORR_EINVAL, "%s: out is NULL", fn);
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    return make_cluster_scope(c, fn, out, [&](orr_index *sh, orr_scope **part) { return orr_scope_create_ticks(sh, ticks_from, ticks_to, part); });
}

int orr_cluster_scope_create_terms(orr_cluster *c, int32_t n_terms, const uint8_t *terms_utf8, const uint32_t *term_off, int32_t mode,
                                   orr_cluster_scope **out)
{
    static const char *fn = "orr_cluster_scope_create_terms";
    if (!out) return fail(ORR_EINVAL, "%s: out is NULL", fn);
    if (!scope_terms::terms_valid(n_terms)) return fail(ORR_EINVAL, "%s: n_terms must be in 0 .. %d", fn, scope_terms::kMaxTerms);
    if (n_terms > 0 && (!terms_utf8 || !term_off)) return fail(ORR_EINVAL, "%s: terms_utf8 or term_off is NULL with %d terms", fn, n_terms);
    if (!scope_terms::mode_valid(mode)) return fail(ORR_EINVAL, "%s: mode must be ORR_TERMS_ALL (0) or ORR_TERMS_ANY (1)", fn);
    const int32_t bad = scope_terms::first_bad_term(term_off, n_terms);
    if (bad >= 0 && term_off[bad + 1] == term_off[bad]) return fail(ORR_EINVAL, "%s: term %d is empty", fn, bad);
    if (bad >= 0) return fail(ORR_EINVAL, "%s: term_off is not monotone at term %d", fn, bad);
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    return make_cluster_scope(c, fn, out, [&](orr_index *sh, orr_scope **part) { return orr_scope_create_terms(sh, n_terms, terms_utf8, term_off, mode, part); });
}

int orr_cluster_scope_create_near(orr_cluster *c, int32_t n_probes, int32_t dim, const float *probes, double min_cosine, int32_t mode,
                                  orr_cluster_scope **out)
{
    static const char *fn = "orr_cluster_scope_create_near";
    ORR_TRY(near_arguments(fn, out == nullptr, n_probes, dim, probes, mode, min_cosine));
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (n_probes > 0 && dim > 0 && is_device_pointer(probes)) return fail(ORR_EINVAL, "%s: probes must be in host memory (every shard's device reads them)", fn);
    return make_cluster_scope(c, fn, out, [&](orr_index *sh, orr_scope **part) { return orr_scope_create_near(sh, n_probes, dim, probes, min_cosine, mode, part); });
}

int orr_cluster_scope_add_ids(orr_cluster_scope *s, int64_t n_ids, const int64_t *ids, int64_t *out_added)
{
    static const char *fn = "orr_cluster_scope_add_ids";
    if (n_ids < 0) return fail(ORR_EINVAL, "%s: n_ids is negative", fn);
    if (n_ids > 0 && !ids) return fail(ORR_EINVAL, "%s: ids is NULL with %lld ids", fn, (long long)n_ids);
    if (!s) return fail(ORR_EINVAL, "%s: null scope", fn);
    if (n_ids > 0 && is_device_pointer(ids)) return fail(ORR_EINVAL, "%s: ids must be in host memory (every shard's device reads them)", fn);
    orr_cluster *c = nullptr;
    ORR_TRY(cluster_scope_owner(s, fn, &c));
    std::shared_lock<std::shared_mutex> lock(c->mu);
    const int32_t G = (int32_t)c->shards.size();
    std::vector<Lane> lanes;
    acquire_cluster_lanes(c, lanes);
    std::vector<std::unique_lock<std::shared_mutex>> held;     // every part exclusively, in ascending shard order
    held.reserve((size_t)G);
    for (int32_t g = 0; g < G; ++g) held.emplace_back(s->parts[(size_t)g]->mu);
    ORR_TRY(cluster_scope_owner(s, fn, &c));
    ORR_TRY(cluster_scope_parts_alive(c, s, fn));
    std::vector<int64_t> added((size_t)G, 0);
    const int r = for_each_shard(G, [&](int32_t g) -> int {
        orr_index *lane = lanes[(size_t)g].lane;
        std::lock_guard<std::mutex> l(lane->mu);
        return scope_add_ids_held(lane, s->parts[(size_t)g], n_ids, ids, &added[(size_t)g]);
    });
    if (r != ORR_OK) {             // some shards may hold the edit and others not: never searched like that
        const std::string keep = g_last_error;
        orphan_cluster_scope(s);
        g_last_error = keep;
        return r;
    }
    if (out_added) { *out_added = 0; for (int64_t a : added) *out_added += a; }
    return ORR_OK;
}

int orr_cluster_scope_combine(orr_cluster_scope *dst, int32_t op, const orr_cluster_scope *src)
{
    static const char *fn = "orr_cluster_scope_combine";
    if (!scope_set::op_valid(op)) return fail(ORR_EINVAL, "%s: op must be ORR_SCOPE_AND (0), ORR_SCOPE_OR (1) or ORR_SCOPE_ANDNOT (2)", fn);
    if (!dst || !src) return fail(ORR_EINVAL, "%s: null scope", fn);
    auto pair = [&](orr_cluster **c) -> int {
        *c = dst->owner.load();
        switch (chandle::pair_valid(*c, src->owner.load(), dst->parts.size(), src->parts.size())) {
        case chandle::Pair::Orphaned: return fail(ORR_ESTATE, "%s: a cluster scope is orphaned: its cluster was destroyed, or an edit of it failed on some shards", fn);
        case chandle::Pair::OtherCluster: return fail(ORR_EINVAL, "%s: the scopes belong to different clusters", fn);
        case chandle::Pair::Shards: return fail(ORR_ESTATE, "%s: the scopes cover different numbers of shards", fn);
        case chandle::Pair::Ok: break;
        }
        return ORR_OK;
    };
    orr_cluster *c = nullptr;
    ORR_TRY(pair(&c));
    std::shared_lock<std::shared_mutex> lock(c->mu);
    const int32_t G = (int32_t)c->shards.size();
    std::vector<Lane> lanes;
    acquire_cluster_lanes(c, lanes);
    // ascending shard; within a shard dst exclusively, src shared, the lower address first (chandle::holds)
    std::vector<uintptr_t> a_dst, a_src;
    for (int32_t g = 0; g < G; ++g) {
        a_dst.push_back(reinterpret_cast<uintptr_t>(dst->parts[(size_t)g]));
        a_src.push_back(reinterpret_cast<uintptr_t>(src->parts[(size_t)g]));
    }
    std::vector<std::unique_lock<std::shared_mutex>> held_w;
    std::vector<std::shared_lock<std::shared_mutex>> held_r;
    held_w.reserve((size_t)G); held_r.reserve((size_t)G);
    for (const chandle::Hold &h : chandle::holds(a_dst, a_src, true)) {
        if (h.exclusive) held_w.emplace_back(dst->parts[(size_t)h.shard]->mu);
        else held_r.emplace_back(src->parts[(size_t)h.shard]->mu);
    }
    ORR_TRY(pair(&c));
    ORR_TRY(cluster_scope_parts_alive(c, dst, fn));
    ORR_TRY(cluster_scope_parts_alive(c, src, fn));
    const int r = for_each_shard(G, [&](int32_t g) -> int {
        orr_index *lane = lanes[(size_t)g].lane;
        std::lock_guard<std::mutex> l(lane->mu);
        return scope_combine_held(lane, dst->parts[(size_t)g], op, src->parts[(size_t)g]);
    });
    if (r != ORR_OK) {             // some shards may hold the edit and others not: never searched like that
        const std::string keep = g_last_error;
        held_w.clear(); held_r.clear();
        orphan_cluster_scope(dst);
        g_last_error = keep;
    }
    return r;
}

int64_t orr_cluster_scope_rows(const orr_cluster_scope *s)
{
    if (!s || !s->owner.load()) return -1;
    int64_t n = 0;
    for (const orr_scope *part : s->parts) {
        const int64_t live = orr_scope_rows(part);
        if (live < 0) return -1;
        n += live;
    }
    return n;
}

int orr_cluster_scope_row_ids(orr_cluster_scope *s, int64_t cap, int64_t *out_ids, int64_t *out_n)
{
    static const char *fn = "orr_cluster_scope_row_ids";
    if (cap < 0) return fail(ORR_EINVAL, "%s: cap is negative", fn);
    if (!out_n) return fail(ORR_EINVAL, "%s: out_n is NULL", fn);
    if (cap > 0 && !out_ids) return fail(ORR_EINVAL, "%s: out_ids is NULL with room for %lld ids", fn, (long long)cap);
    if (!s) return fail(ORR_EINVAL, "%s: null scope", fn);
    orr_cluster *c = nullptr;
    ORR_TRY(cluster_scope_owner(s, fn, &c));
    std::shared_lock<std::shared_mutex> lock(c->mu);
    const int32_t G = (int32_t)c->shards.size();
    std::vector<Lane> lanes;
    acquire_cluster_lanes(c, lanes);
    std::vector<std::shared_lock<std::shared_mutex>> held;
    held.reserve((size_t)G);
    for (int32_t g = 0; g < G; ++g) held.emplace_back(s->parts[(size_t)g]->mu);
    ORR_TRY(cluster_scope_owner(s, fn, &c));
    ORR_TRY(cluster_scope_parts_alive(c, s, fn));
    std::vector<int64_t> live((size_t)G);
    for (int32_t g = 0; g < G; ++g) live[(size_t)g] = s->parts[(size_t)g]->live.load();
    const chandle::RowIdPlan plan = chandle::row_id_plan(live, cap);
    *out_n = plan.total;
    if (!plan.fits) return fail(ORR_EINVAL, "%s: the scope holds %lld rows, out_ids has room for %lld", fn, (long long)plan.total, (long long)cap);
    return for_each_shard(G, [&](int32_t g) -> int {
        if (live[(size_t)g] <= 0) return ORR_OK;
        orr_index *lane = lanes[(size_t)g].lane;
        std::lock_guard<std::mutex> l(lane->mu);
        return scope_row_ids_held(lane, s->parts[(size_t)g], live[(size_t)g], out_ids + plan.offset[(size_t)g]);
    });
}

const orr_scope *orr_cluster_scope_shard(const orr_cluster_scope *s, int32_t i)
{
    if (!s || i < 0 || i >= (int32_t)s->parts.size()) { (void)fail(ORR_EINVAL, "orr_cluster_scope_shard: no shard %d", i); return nullptr; }
    return s->parts[(size_t)i];
}

void orr_cluster_scope_destroy(orr_cluster_scope *s)
{
    if (!s) return;
    {   // (the cluster is not destroyed meanwhile; afterwards it no longer knows this scope)
        std::lock_guard<std::mutex> life(g_scope_life_mu);
        orr_cluster *c = s->owner.load();
        if (c) c->cscopes.erase(std::remove(c->cscopes.begin(), c->cscopes.end(), s), c->cscopes.end());
        s->owner.store(nullptr);
    }
    for (orr_scope *part : s->parts) orr_scope_destroy(part);      // each against its own shard's destroy, as a single scope
    delete s;
}

int orr_cluster_search_batch_in_scope(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const uint8_t *terms_utf8,
                                      const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                      int64_t candidate_limit, const orr_cluster_scope *scope, int64_t *out_rows, double *out_scores,
                                      int32_t *out_counts)
{
    static const char *fn = "orr_cluster_search_batch_in_scope";
    const BatchArgs a{B, dim, q_host, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    if (B <= 0) return fail(ORR_EINVAL, "%s: batch size must be positive", fn);
    if (dim < 0) return fail(ORR_EINVAL, "%s: negative query dimension", fn);
    if (dim > 0 && !q_host) return fail(ORR_EINVAL, "%s: q is NULL with dim %d", fn, dim);
    if (!query_term_off) return fail(ORR_EINVAL, "%s: query_term_off is required", fn);
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "%s: output buffers are required", fn);
    if (!scope) return fail(ORR_EINVAL, "%s: null scope", fn);
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (dim > 0 && is_device_pointer(q_host)) return fail(ORR_EINVAL, "%s: the query vectors must be in host memory (every shard's device reads them)", fn);
    std::shared_lock<std::shared_mutex> lock(c->mu);   // searches run side by side; seal and destroy are exclusive
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    orr_cluster *own = nullptr;
    ORR_TRY(cluster_scope_owner(scope, fn, &own));
    if (own != c || scope->parts.size() != c->shards.size()) return fail(ORR_EINVAL, "%s: the scope belongs to another cluster", fn);
    ClusterScope cs{true, 0, nullptr, nullptr};
    cs.handle = scope;
    return cluster_scope_search(c, fn, a, cs, out_rows, out_scores, out_counts);
}

int orr_cluster_search_batch_in_scopes(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const uint8_t *terms_utf8,
                                       const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                       int64_t candidate_limit, int32_t n_scopes, const orr_cluster_scope *const *scopes,
                                       const int32_t *query_scope, int64_t *out_rows, double *out_scores, int32_t *out_counts)
{
    static const char *fn = "orr_cluster_search_batch_in_scopes";
    const BatchArgs a{B, dim, q_host, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    if (!scope_set::scopes_valid(n_scopes)) return fail(ORR_EINVAL, "%s: n_scopes must be in 1 .. %d", fn, scope_set::kMaxScopes);
    if (!scopes) return fail(ORR_EINVAL, "%s: scopes is NULL", fn);
    for (int32_t g = 0; g < n_scopes; ++g)
        if (!scopes[g]) return fail(ORR_EINVAL, "%s: scopes[%d] is a null scope", fn, g);
    if (!query_scope) return fail(ORR_EINVAL, "%s: query_scope is NULL", fn);
    if (B > 0 && !group::assignment_valid(query_scope, B, n_scopes))
        return fail(ORR_EINVAL, "%s: query_scope must name a scope in 0 .. %d for every query", fn, n_scopes - 1);
    if (B <= 0) return fail(ORR_EINVAL, "%s: batch size must be positive", fn);
    if (dim < 0) return fail(ORR_EINVAL, "%s: negative query dimension", fn);
    if (dim > 0 && !q_host) return fail(ORR_EINVAL, "%s: q is NULL with dim %d", fn, dim);
    if (!query_term_off) return fail(ORR_EINVAL, "%s: query_term_off is required", fn);
    if (!out_rows || !out_scores) return fail(ORR_EINVAL, "%s: output buffers are required", fn);
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (dim > 0 && is_device_pointer(q_host)) return fail(ORR_EINVAL, "%s: the query vectors must be in host memory (every shard's device reads them)", fn);
    std::shared_lock<std::shared_mutex> lock(c->mu);   // searches run side by side; seal and destroy are exclusive
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    for (int32_t g = 0; g < n_scopes; ++g) {
        orr_cluster *own = nullptr;
        ORR_TRY(cluster_scope_owner(scopes[g], fn, &own));
        if (own != c || scopes[g]->parts.size() != c->shards.size()) return fail(ORR_EINVAL, "%s: scopes[%d] belongs to another cluster", fn, g);
    }
    return cluster_grouped_search(c, fn, a, n_scopes, scopes, query_scope, out_rows, out_scores, out_counts);
}

// Every shard runs the single call at once, each on a lane of its own; the host merges the shards' lists by (cosine descending,
// order_key ascending), sums the totals and cuts at max_hits.  The limit met on any shard is the call's: the upper bounds summed.
static int cluster_range_search(orr_cluster *c, const RangeArgs &a, const orr_cluster_scope *within, orr_range_hit *out_hits, int32_t *out_n, int64_t *out_total)
{
    const char *fn = a.fn;
    const int32_t B = a.B, dim = a.dim, max_hits = a.max_hits;
    const float *q_host = a.q;
    ORR_TRY(range_arguments(fn, a, out_hits, out_n, out_total));
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (B == 0) return ORR_OK;
    if (dim > 0 && is_device_pointer(q_host)) return fail(ORR_EINVAL, "%s: the query vectors must be in host memory (every shard's device reads them)", fn);
    std::shared_lock<std::shared_mutex> lock(c->mu);   // like a search: beside the others; seal and destroy are exclusive
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    auto scope_of_this_cluster = [&]() -> int {
        orr_cluster *own = nullptr;
        ORR_TRY(cluster_scope_owner(within, fn, &own));
        if (own != c || within->parts.size() != c->shards.size()) return fail(ORR_EINVAL, "%s: the scope belongs to another cluster", fn);
        return ORR_OK;
    };
    if (within) ORR_TRY(scope_of_this_cluster());
    const int32_t G = (int32_t)c->shards.size();
    std::vector<Lane> lanes;
    acquire_cluster_lanes(c, lanes);
    std::vector<std::shared_lock<std::shared_mutex>> held;     // every part shared, in ascending shard order
    if (within) {
        held.reserve((size_t)G);
        for (int32_t g = 0; g < G; ++g) held.emplace_back(within->parts[(size_t)g]->mu);
        ORR_TRY(scope_of_this_cluster());
        ORR_TRY(cluster_scope_parts_alive(c, within, fn));
    }
    std::vector<RangeOut> outs((size_t)G);
    ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
        orr_index *lane = lanes[(size_t)g].lane;
        std::lock_guard<std::mutex> l(lane->mu);
        const orr_scope *part = within ? within->parts[(size_t)g] : nullptr;
        if (part && part->n_rows != lane->n_rows)
            return fail(ORR_ESTATE, "%s: the scope covers %lld rows of shard %d, the shard holds %lld", fn, (long long)part->n_rows, g, (long long)lane->n_rows);
        return range_on_lane(lane, a, part, outs[(size_t)g]);
    }));
    RangeOut o;
    o.hits.assign((size_t)B, {});
    o.total.assign((size_t)B, 0);
    for (const RangeOut &part : outs) o.limit = o.limit || part.limit;
    for (int32_t b = 0; b < B; ++b) {
        std::vector<const std::vector<range::Hit> *> lists;
        for (const RangeOut &part : outs) {
            o.total[(size_t)b] += part.total[(size_t)b];
            lists.push_back(&part.hits[(size_t)b]);
        }
        if (!o.limit) o.hits[(size_t)b] = range::merge_lists(lists, max_hits);
    }
    return range_write(fn, a, o, out_hits, out_n, out_total);
}

int orr_cluster_search_range_cosine(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const double *min_cosine,
                                    const orr_cluster_scope *within, int32_t max_hits, orr_range_hit *out_hits, int32_t *out_n, int64_t *out_total)
{
    return cluster_range_search(c, RangeArgs{B, dim, q_host, min_cosine, max_hits, false, "orr_cluster_search_range_cosine"}, within, out_hits, out_n, out_total);
}

int orr_cluster_search_range_cosine_bulk(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const double *min_cosine,
                                         const orr_cluster_scope *within, int32_t max_hits, orr_range_hit *out_hits, int32_t *out_n, int64_t *out_total)
{
    return cluster_range_search(c, RangeArgs{B, dim, q_host, min_cosine, max_hits, true, "orr_cluster_search_range_cosine_bulk"}, within, out_hits, out_n, out_total);
}

}  // extern "C"

// ---- diverse search over the shards (orr_cluster_search_batch_diverse, orr_cluster_pair_dots) -------------------------------
// The pool is the cluster's plain search (the in-scope search with a scope) for topk = pool, unchanged, which hands back every
// result's order_key through BatchArgs::out_keys; the cosine and the greedy pass are the single index's (orr_diverse_plan.h).
// What lies between is the pair step: the two rows of a pair may lie on different shards, and orr_cluster_diverse_plan.h says
// which rows go where.  Per group of the plan, on the lanes the call holds:
//   1. every source shard at once: ONE rows_gather of its listed positions into a dense buffer, which goes to pinned host memory;
//   2. every home shard at once: the runs meant for it go from the sources' pinned buffers into its staging buffer on its own
//      stream, then ONE two-source pair-dot launch over its lists, and the matrices come back.
// Nothing here reads another device's memory from a kernel; the rows travel as the records of a cluster search do by default.

namespace {

// The pair matrices of the plan's lists, mats [lists][stride][stride] (the elements at or beyond a list's length are not set).
int cluster_pair_step(orr_cluster *c, std::vector<Lane> &lanes, const cdiverse::Plan &plan, std::vector<double> &mats)
{
    const int32_t G = (int32_t)c->shards.size(), stride = plan.stride;
    const size_t per_mat = (size_t)stride * (size_t)stride, row_bytes = sizeof(float) * (size_t)c->dim;
    mats.assign(plan.lists.size() * per_mat, 0.0);
    for (const cdiverse::Group &grp : plan.groups) {
        // ---- the sources: gather, then down to pinned memory
        ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
            const std::vector<uint32_t> &want = grp.gather[(size_t)g];
            if (want.empty()) return ORR_OK;
            orr_index *lane = lanes[(size_t)g].lane;
            std::lock_guard<std::mutex> lock(lane->mu);
            for (uint32_t p : want)                                           // before the launch: the kernel is never handed a row it cannot read
                if ((int64_t)p >= lane->n_rows) return fail(ORR_EDEVICE, "orr_cluster: the pair step lists position %u of shard %d, which holds %lld rows", p, g, (long long)lane->n_rows);
            ORR_TRY(bind_device(lane));
            hipStream_t s = lane->stream;
            const size_t n = want.size(), rows_at = (sizeof(uint32_t) * n + 15) / 16 * 16;
            ORR_TRY(lane->ws_diverse_gpos.reserve(sizeof(uint32_t) * n));
            ORR_TRY(lane->ws_diverse_gather.reserve(row_bytes * n));
            ORR_TRY(lane->pin_diverse_rows.reserve(rows_at + row_bytes * n));
            uint8_t *pin = lane->pin_diverse_rows.as<uint8_t>();
            memcpy(pin, want.data(), sizeof(uint32_t) * n);
            HIP_TRY(hipMemcpyAsync(lane->ws_diverse_gpos.p, pin, sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
            {
                Timed t(lane, "rows_gather", 8.0 * (double)c->dim * (double)n);
                HIP_TRY(orr::launch_rows_gather(lane->d_emb, lane->n_rows, c->dim, lane->ws_diverse_gpos.as<uint32_t>(), (int64_t)n, lane->ws_diverse_gather.as<float>(), s));
            }
            HIP_TRY(hipMemcpyAsync(pin + rows_at, lane->ws_diverse_gather.p, row_bytes * n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            collect_events(lane);
            return ORR_OK;
        }));
        // ---- the homes: the runs up into the staging buffer, then the dots
        ORR_TRY(for_each_shard(G, [&](int32_t h) -> int {
            const std::vector<int32_t> &mine = grp.lists[(size_t)h];
            if (mine.empty()) return ORR_OK;
            orr_index *lane = lanes[(size_t)h].lane;
            std::lock_guard<std::mutex> lock(lane->mu);
            ORR_TRY(bind_device(lane));
            ORR_TRY(lane->ws_diverse_foreign.reserve(std::max<size_t>(row_bytes * (size_t)grp.staged[(size_t)h], 16)));
            for (const cdiverse::Run &run : grp.runs) {
                if (run.home != h) continue;
                const orr_index *src = lanes[(size_t)run.src].lane;       // (held by this call: nobody writes its pinned buffer now)
                const size_t rows_at = (sizeof(uint32_t) * grp.gather[(size_t)run.src].size() + 15) / 16 * 16;
                HIP_TRY(hipMemcpyAsync(lane->ws_diverse_foreign.as<uint8_t>() + row_bytes * (size_t)run.home_at,
                                       src->pin_diverse_rows.as<uint8_t>() + rows_at + row_bytes * (size_t)run.src_at, row_bytes * (size_t)run.rows,
                                       hipMemcpyHostToDevice, lane->stream));
            }
            const size_t nl = mine.size();
            std::vector<uint32_t> pos(nl * (size_t)stride, 0u), cnt(nl, 0u);
            std::vector<uint64_t> foreign(nl, 0);
            for (size_t i = 0; i < nl; ++i) {
                const cdiverse::List &l = plan.lists[(size_t)mine[i]];
                cnt[i] = (uint32_t)l.n;
                foreign[i] = l.foreign;
                for (int32_t k = 0; k < l.n; ++k) {
                    const int64_t limit = ((l.foreign >> k) & 1) ? grp.staged[(size_t)h] : lane->n_rows;
                    if ((int64_t)l.at[(size_t)k] >= limit) return fail(ORR_EDEVICE, "orr_cluster: the pair step lists row %u of shard %d beyond its %lld rows", l.at[(size_t)k], h, (long long)limit);
                    pos[i * (size_t)stride + (size_t)k] = l.at[(size_t)k];
                }
            }
            std::vector<double> got(nl * per_mat);
            ORR_TRY(pair_dots_on_lane(lane, (int32_t)nl, stride, pos.data(), cnt.data(), got.data(), foreign.data(), grp.staged[(size_t)h]));   // (its stream: behind the copies)
            for (size_t i = 0; i < nl; ++i) memcpy(mats.data() + (size_t)mine[i] * per_mat, got.data() + i * per_mat, sizeof(double) * per_mat);
            return ORR_OK;
        }));
    }
    return ORR_OK;
}

// where the shards lie in the global candidate order, read from the lanes the call holds
void cluster_extents(const std::vector<Lane> &lanes, std::vector<int64_t> &base, std::vector<int64_t> &rows)
{
    for (const Lane &ln : lanes) { base.push_back(ln.lane->row_base); rows.push_back(ln.lane->n_rows); }
}

int cluster_scope_of(const orr_cluster *c, const orr_cluster_scope *s, const char *fn)
{
    orr_cluster *own = nullptr;
    ORR_TRY(cluster_scope_owner(s, fn, &own));
    if (own != c || s->parts.size() != c->shards.size()) return fail(ORR_EINVAL, "%s: the scope belongs to another cluster", fn);
    return ORR_OK;
}

}  // namespace

extern "C" {

int orr_cluster_search_batch_diverse(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const uint8_t *terms_utf8,
                                     const uint32_t *term_off, const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                     int64_t candidate_limit, const orr_cluster_scope *within, int32_t pool, int32_t mode, double param,
                                     int64_t *out_rows, double *out_scores, int32_t *out_counts, int32_t *out_pool_rank)
{
    static const char *fn = "orr_cluster_search_batch_diverse";
    switch (diverse::first_invalid(!out_rows || !out_scores || !out_counts, topk, pool, mode, param)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out_rows, out_scores and out_counts are required", fn);
    case 2: return fail(ORR_EINVAL, "%s: pool must be in 1 .. %d", fn, diverse::kMaxPool);
    case 3: return fail(ORR_EINVAL, "%s: topk %d exceeds the pool of %d", fn, topk, pool);
    case 4: return fail(ORR_EINVAL, "%s: mode must be ORR_DIVERSE_COLLAPSE (0) or ORR_DIVERSE_MMR (1)", fn);
    case 5: return fail(ORR_EINVAL, "%s: param is NaN", fn);
    default: return fail(ORR_EINVAL, "%s: lambda must be in [0, 1]", fn);
    }
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (B == 0) return ORR_OK;
    std::shared_lock<std::shared_mutex> lock(c->mu);   // from the pool's search to the last matrix: no compaction or insertion moves a row in between
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    if (within) ORR_TRY(cluster_scope_of(c, within, fn));
    // ---- the pool: the cluster's own search for topk = pool, with each result's order_key
    const int32_t take = diverse::take_of(topk);
    BatchArgs pa{B, dim, q_host, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, pool};
    ORR_TRY(check_batch(c->shards[0], pa, fn));
    if (dim > 0 && is_device_pointer(q_host)) return fail(ORR_EINVAL, "%s: the query vectors must be in host memory (every shard's device reads them)", fn);
    std::vector<int64_t> p_rows((size_t)B * pool, -1), keys((size_t)B * pool, -1);
    std::vector<double> p_scores((size_t)B * pool, 0.0);
    std::vector<int32_t> p_cnt((size_t)B, 0);
    pa.out_keys = keys.data();
    std::vector<Lane> lanes;                            // one per shard, ascending: with a scope from the pool's search on, else for the pair step
    if (within) {
        ClusterScope cs{true, 0, nullptr, nullptr};
        cs.handle = within;
        cluster_scope_begin(c, pa, p_rows.data(), p_scores.data(), p_cnt.data());
        cluster_scope_lanes(c, lanes);
        ORR_TRY(cluster_scope_on_lanes(c, fn, pa, cs, lanes, false, false, p_rows.data(), p_scores.data(), p_cnt.data()));
    } else {
        ORR_TRY(cluster_plain_search(c, pa, p_rows.data(), p_scores.data(), p_cnt.data()));
    }
    // ---- the pair step: only the queries whose greedy pass reads a cosine
    std::vector<uint8_t> needs((size_t)B, 0);
    bool any = false;
    for (int32_t b = 0; b < B; ++b) any = (needs[(size_t)b] = diverse::needs_dots(mode, param, p_cnt[(size_t)b], c->dim)) || any;
    cdiverse::Plan plan;
    std::vector<double> mats;
    if (any) {
        if (lanes.empty()) acquire_cluster_lanes(c, lanes);
        std::vector<int64_t> base, rows;
        cluster_extents(lanes, base, rows);
        plan = cdiverse::make_plan(base, rows, B, pool, keys.data(), p_cnt.data(), needs.data(), c->dim);
        if (!plan.ok) return fail(ORR_EDEVICE, "%s: query %d's result with order_key %lld lies outside every shard", fn, plan.bad_query, (long long)plan.bad_key);
        ORR_TRY(cluster_pair_step(c, lanes, plan, mats));
    }
    lanes.clear();
    // ---- the greedy pass and the outputs, as on one index
    const int32_t stride = plan.stride;
    std::vector<int32_t> picks((size_t)take);
    for (int32_t b = 0; b < B; ++b) {
        const int32_t n = p_cnt[(size_t)b], l = any ? plan.list_of[(size_t)b] : -1;
        const double *m = l >= 0 ? mats.data() + (size_t)l * stride * stride : nullptr;
        auto cosine = [m, stride](int32_t i, int32_t j) -> double {
            if (!m) return 0.0;
            return scope_near::cosine_of(m[diverse::mat_index(stride, i, j)], m[diverse::mat_index(stride, i, i)], m[diverse::mat_index(stride, j, j)]);
        };
        const int32_t kept = mode == diverse::Collapse ? diverse::select_collapse(n, take, param, cosine, picks.data())
                                                       : diverse::select_mmr(n, take, param, p_scores.data() + (size_t)b * pool, cosine, picks.data());
        for (int32_t i = 0; i < take; ++i) {
            const size_t o = (size_t)b * take + i;
            const bool have = i < kept;
            out_rows[o] = have ? p_rows[(size_t)b * pool + picks[(size_t)i]] : -1;
            out_scores[o] = have ? p_scores[(size_t)b * pool + picks[(size_t)i]] : 0.0;
            if (out_pool_rank) out_pool_rank[o] = have ? picks[(size_t)i] : -1;
        }
        out_counts[b] = kept;
    }
    return ORR_OK;
}

int orr_cluster_pair_dots(orr_cluster *c, int32_t n_lists, const uint32_t *list_off, const int64_t *order_keys, int32_t stride, double *out)
{
    static const char *fn = "orr_cluster_pair_dots";
    switch (diverse::first_invalid_pairs(!out, n_lists, !list_off, !order_keys, stride)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out is NULL", fn);
    case 2: return fail(ORR_EINVAL, "%s: n_lists is negative", fn);
    case 3: return fail(ORR_EINVAL, "%s: stride must be in 1 .. %d", fn, diverse::kMaxPool);
    case 4: return fail(ORR_EINVAL, "%s: list_off is NULL", fn);
    default: return fail(ORR_EINVAL, "%s: order_keys is NULL", fn);
    }
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (list_off[0] != 0) return fail(ORR_EINVAL, "%s: list_off must start at 0", fn);
    for (int32_t l = 0; l < n_lists; ++l) {
        if (list_off[l + 1] < list_off[l]) return fail(ORR_EINVAL, "%s: list_off decreases at list %d", fn, l);
        if (list_off[l + 1] - list_off[l] > (uint32_t)stride) return fail(ORR_EINVAL, "%s: list %d holds %u order keys, stride is %d", fn, l, list_off[l + 1] - list_off[l], stride);
    }
    std::shared_lock<std::shared_mutex> lock(c->mu);
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    std::vector<Lane> lanes;
    acquire_cluster_lanes(c, lanes);
    std::vector<int64_t> base, rows;
    cluster_extents(lanes, base, rows);
    for (uint32_t e = 0; e < list_off[n_lists]; ++e) {                        // before any launch
        cdiverse::Place pl;
        if (!cdiverse::locate(base, rows, order_keys[e], &pl)) return fail(ORR_EINVAL, "%s: order_keys[%u] = %lld is outside every shard", fn, e, (long long)order_keys[e]);
    }
    if (n_lists == 0) return ORR_OK;
    std::vector<int64_t> keys((size_t)n_lists * stride, -1);
    std::vector<int32_t> cnt((size_t)n_lists, 0);
    std::vector<uint8_t> needs((size_t)n_lists, 0);
    for (int32_t l = 0; l < n_lists; ++l) {
        cnt[(size_t)l] = (int32_t)(list_off[l + 1] - list_off[l]);
        needs[(size_t)l] = c->dim > 0 && cnt[(size_t)l] > 0;
        for (int32_t i = 0; i < cnt[(size_t)l]; ++i) keys[(size_t)l * stride + i] = order_keys[list_off[l] + (uint32_t)i];
    }
    const cdiverse::Plan plan = cdiverse::make_plan(base, rows, n_lists, stride, keys.data(), cnt.data(), needs.data(), c->dim);
    if (!plan.ok) return fail(ORR_EINVAL, "%s: order key %lld of list %d is outside every shard", fn, (long long)plan.bad_key, plan.bad_query);
    std::vector<double> mats;
    ORR_TRY(cluster_pair_step(c, lanes, plan, mats));
    for (int32_t l = 0; l < n_lists; ++l) {                                   // (what lies at or beyond a list's length stays as the caller left it)
        const int32_t at = plan.list_of[(size_t)l];
        for (int32_t i = 0; i < cnt[(size_t)l]; ++i) {
            double *dst = out + ((size_t)l * stride + i) * stride;
            if (at < 0) { for (int32_t j = 0; j < cnt[(size_t)l]; ++j) dst[j] = 0.0; continue; }          // a cluster without a dimension: zero rows
            memcpy(dst, mats.data() + ((size_t)at * plan.stride + i) * plan.stride, sizeof(double) * cnt[(size_t)l]);
        }
    }
    return ORR_OK;
}

}  // extern "C"

// ---- row keys and the per-key search over the shards (orr_cluster_keys, orr_cluster_search_batch_per_key) ---------------------
// The answer, the rounds, the walk and the union table are the single index's (orr_per_key_plan.h, per_key_run above); the
// device work is the single index's kernels, run on every shard at once (per_key_gather, per_key_freeze, per_key_slice_scopes).
// What the cluster adds is orr_cluster_per_key_plan.h's: which shard gathers which pool members, the seen order keys as each
// shard's local positions, each shard's share of the limit, the order of the holds.  A key closes cluster-wide: the slice's
// union table goes to every shard as it is.

namespace {

// The cluster of a cluster keys handle, or ORR_ESTATE: orphaned.
int cluster_keys_owner(const orr_cluster_keys *k, const char *fn, orr_cluster **c)
{
    *c = k->owner.load();
    if (!*c) return fail(ORR_ESTATE, "%s: the cluster keys are orphaned: their cluster was destroyed, or an edit of them failed on some shards", fn);
    return ORR_OK;
}

// Every part belongs to its shard of `c` still (none was orphaned on its own); the caller holds the parts.
int cluster_keys_parts_alive(const orr_cluster *c, const orr_cluster_keys *k, const char *fn)
{
    for (size_t g = 0; g < k->parts.size(); ++g) {
        orr_index *own = nullptr;
        ORR_TRY(keys_owner(k->parts[g], c->shards[g], fn, &own));
    }
    return ORR_OK;
}

void orphan_cluster_keys(orr_cluster_keys *k)
{
    std::lock_guard<std::mutex> life(g_scope_life_mu);
    orr_cluster *c = k->owner.load();
    if (!c) return;
    c->ckeys.erase(std::remove(c->ckeys.begin(), c->ckeys.end(), k), c->ckeys.end());
    k->owner.store(nullptr);
}

// What the shards of a cluster per-key call own from its first gather on; each is released with its shard's device bound.
struct ClusterPerKeyWork {
    std::vector<std::unique_ptr<PerKeyWork>> w;
    std::vector<int> device;
    explicit ClusterPerKeyWork(const orr_cluster *c)
    {
        for (const orr_index *sh : c->shards) { w.emplace_back(new PerKeyWork()); device.push_back(sh->device); }
    }
    ~ClusterPerKeyWork()
    {
        for (size_t g = 0; g < w.size(); ++g) { (void)hipSetDevice(device[g]); w[g].reset(); }
    }
};

// orr_cluster_search_batch_per_key behind its checks, the cluster held shared.
int cluster_per_key_run(orr_cluster *c, const char *fn, const BatchArgs &a, const orr_cluster_scope *within, const orr_cluster_keys *keys,
                        int32_t max_per_key, int32_t pool, int64_t *out_rows, double *out_scores, int64_t *out_row_keys, int32_t *out_counts,
                        int32_t *out_rounds)
{
    const int32_t G = (int32_t)c->shards.size(), B = a.B, take = per_key::take_of(a.topk);
    for (size_t i = 0; i < (size_t)B * take; ++i) { out_rows[i] = -1; out_scores[i] = 0.0; out_row_keys[i] = ORR_KEY_NONE; }
    for (int32_t b = 0; b < B; ++b) { out_counts[b] = 0; if (out_rounds) out_rounds[b] = 0; }
    std::vector<int64_t> r_rows((size_t)B * pool, -1), r_keys((size_t)B * pool, -1);    // r_keys: each result's global order key
    std::vector<double> r_scores((size_t)B * pool, 0.0);
    std::vector<int32_t> r_cnt((size_t)B, 0);
    // ONE set of lanes (ascending shard order) for everything behind round 1, with a scope from round 1 on; behind the lanes the
    // keys' and the scope's parts shared, in the one order of cper_key::holds.  The call never takes a second set.
    std::vector<Lane> lanes;
    std::vector<std::shared_lock<std::shared_mutex>> held;
    auto hold_parts = [&]() -> int {
        std::vector<uintptr_t> ka, sa;
        for (int32_t g = 0; g < G; ++g) {
            ka.push_back(reinterpret_cast<uintptr_t>(keys->parts[(size_t)g]));
            if (within) sa.push_back(reinterpret_cast<uintptr_t>(within->parts[(size_t)g]));
        }
        const std::vector<cper_key::Hold> order = cper_key::holds(ka, sa);
        held.reserve(order.size());
        for (const cper_key::Hold &h : order) {
            if (h.which) held.emplace_back(within->parts[(size_t)h.shard]->mu);
            else held.emplace_back(keys->parts[(size_t)h.shard]->mu);
        }
        orr_cluster *own = nullptr;
        ORR_TRY(cluster_keys_owner(keys, fn, &own));
        ORR_TRY(cluster_keys_parts_alive(c, keys, fn));
        for (int32_t g = 0; g < G; ++g)
            if (keys->parts[(size_t)g]->n_rows != lanes[(size_t)g].lane->n_rows)
                return fail(ORR_ESTATE, "%s: the keys cover %lld rows of shard %d, the shard holds %lld", fn, (long long)keys->parts[(size_t)g]->n_rows, g,
                            (long long)lanes[(size_t)g].lane->n_rows);
        if (within) {
            ORR_TRY(cluster_scope_owner(within, fn, &own));
            ORR_TRY(cluster_scope_parts_alive(c, within, fn));
        }
        return ORR_OK;
    };
    // ---- round 1: the pool, exactly the call the cluster's diverse search makes for its own
    {
        BatchArgs pa = a;
        pa.topk = pool;
        pa.out_keys = r_keys.data();
        if (within) {
            ClusterScope cs{true, 0, nullptr, nullptr};
            cs.handle = within;
            cluster_scope_begin(c, pa, r_rows.data(), r_scores.data(), r_cnt.data());
            cluster_scope_lanes(c, lanes);
            ORR_TRY(hold_parts());
            ORR_TRY(cluster_scope_on_lanes(c, fn, pa, cs, lanes, true, false, r_rows.data(), r_scores.data(), r_cnt.data()));
        } else {
            ORR_TRY(cluster_plain_search(c, pa, r_rows.data(), r_scores.data(), r_cnt.data()));
            cluster_scope_lanes(c, lanes);
            ORR_TRY(hold_parts());
        }
    }
    std::vector<int64_t> base, rows;
    cluster_extents(lanes, base, rows);
    int64_t all_rows = 0;
    for (int64_t r : rows) all_rows += r;
    ClusterPerKeyWork work(c);
    std::vector<per_key::State> st((size_t)B);          // (State::seen holds global order keys here)
    std::vector<int32_t> ids((size_t)B);                // the queries of the round in flight: [i] of r_* is query ids[i]
    std::iota(ids.begin(), ids.end(), 0);
    bool frozen = false;
    for (int32_t round = 1; !ids.empty(); ++round) {
        if (round > take) return fail(ORR_EDEVICE, "%s: a round kept no row", fn);      // (every round keeps at least one)
        // ---- the round's keys: every shard that holds a member reads its own members' keys with ONE keys_gather
        const size_t nq = ids.size();
        const cper_key::Gather gp = cper_key::gather_plan(base, rows, (int32_t)nq, pool, r_keys.data(), r_cnt.data());
        if (!gp.ok) return fail(ORR_EDEVICE, "%s: a result with order_key %lld lies outside every shard", fn, (long long)gp.bad_key);
        std::vector<int64_t> rk(nq * (size_t)pool, ORR_KEY_NONE);
        ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
            const std::vector<int64_t> &pos = gp.pos[(size_t)g];
            if (pos.empty()) return ORR_OK;
            orr_index *lane = lanes[(size_t)g].lane;
            std::lock_guard<std::mutex> lock(lane->mu);
            for (int64_t p : pos)                                             // before the launch: the kernel is never handed a row it cannot read
                if (p < 0 || p >= lane->n_rows) return fail(ORR_EDEVICE, "%s: the gather lists position %lld of shard %d, which holds %lld rows", fn, (long long)p, g, (long long)lane->n_rows);
            ORR_TRY(bind_device(lane));
            std::vector<int64_t> got;
            ORR_TRY(per_key_gather(lane, keys->parts[(size_t)g], work.w[(size_t)g]->gio, pos, got));
            for (size_t i = 0; i < pos.size(); ++i) rk[(size_t)gp.at[(size_t)g][i]] = got[i];
            return ORR_OK;
        }));
        // ---- the walk
        std::vector<int32_t> unfinished;
        std::vector<int32_t> number((size_t)pool);
        std::iota(number.begin(), number.end(), 0);
        for (size_t i = 0; i < nq; ++i) {
            const int32_t b = ids[i];
            per_key::State &s = st[(size_t)b];
            const size_t had = s.kept.size();
            per_key::walk_round(s, r_cnt[i], rk.data() + i * pool, r_keys.data() + i * pool, number.data(), take, max_per_key, pool);
            for (size_t t = had; t < s.kept.size(); ++t) {
                const size_t o = (size_t)b * take + t, from = i * pool + (size_t)s.kept[t];
                out_rows[o] = r_rows[from]; out_scores[o] = r_scores[from]; out_row_keys[o] = rk[from];
            }
            out_counts[b] = (int32_t)s.kept.size();
            if (out_rounds) out_rounds[b] = s.rounds;
            if (!s.finished) {
                if (s.kept.size() == had) return fail(ORR_EDEVICE, "%s: a round kept no row", fn);
                unfinished.push_back(b);
            }
        }
        if (unfinished.empty()) break;
        // ---- the frozen set, once: on every shard its part of the rows that took part in round 1
        if (!frozen) {
            std::vector<int64_t> took((size_t)G, -1);
            if (within) {
                std::vector<int64_t> live((size_t)G);
                for (int32_t g = 0; g < G; ++g) live[(size_t)g] = within->parts[(size_t)g]->live.load();
                const cscope::Split split = cscope::split_limit(live, a.candidate_limit);
                for (int32_t g = 0; g < G; ++g) {
                    const cper_key::Share sh = cper_key::scope_share(split, g, live[(size_t)g]);
                    took[(size_t)g] = sh.part == cper_key::Part::Empty ? 0 : sh.took;
                }
            }
            ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
                orr_index *lane = lanes[(size_t)g].lane;
                if (lane->n_rows <= 0) return ORR_OK;
                std::lock_guard<std::mutex> lock(lane->mu);
                ORR_TRY(bind_device(lane));
                return per_key_freeze(lane, a, within ? within->parts[(size_t)g] : nullptr, *work.w[(size_t)g], took[(size_t)g]);
            }));
            frozen = true;
        }
        // ---- the next round, in slices of at most 64 queries
        const size_t nu = unfinished.size();
        std::vector<int64_t> n_rows(nu * (size_t)pool, -1), n_keys(nu * (size_t)pool, -1);
        std::vector<double> n_scores(nu * (size_t)pool, 0.0);
        std::vector<int32_t> n_cnt(nu, 0);
        for (size_t b0 = 0; b0 < nu; b0 += (size_t)per_key::kMaxSlots) {
            const int32_t S = (int32_t)std::min<size_t>((size_t)per_key::kMaxSlots, nu - b0);
            const std::vector<int32_t> slice(unfinished.begin() + b0, unfinished.begin() + b0 + S);
            std::vector<const std::set<int64_t> *> closed((size_t)S);
            std::vector<const std::vector<int64_t> *> seen((size_t)S);
            for (int32_t i = 0; i < S; ++i) { closed[(size_t)i] = &st[(size_t)slice[(size_t)i]].closed; seen[(size_t)i] = &st[(size_t)slice[(size_t)i]].seen; }
            std::vector<int64_t> tk;                    // the SAME table on every shard: a key closes cluster-wide
            std::vector<uint64_t> tm;
            per_key::build_table(closed, tk, tm);
            std::vector<std::unique_ptr<orr_scope[]>> tmp((size_t)G);
            ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
                orr_index *lane = lanes[(size_t)g].lane;
                if (lane->n_rows <= 0) {                // an empty shard: empty parts, nothing launched
                    tmp[(size_t)g].reset(new orr_scope[(size_t)S]);
                    for (int32_t i = 0; i < S; ++i) tmp[(size_t)g][(size_t)i].owner.store(const_cast<orr_index *>(owner_of(lane)));
                    return ORR_OK;
                }
                std::lock_guard<std::mutex> lock(lane->mu);
                ORR_TRY(bind_device(lane));
                const cper_key::Seen mine = cper_key::seen_of_shard(base[(size_t)g], rows[(size_t)g], seen);
                return per_key_slice_scopes(lane, keys->parts[(size_t)g], S, tk, tm, mine.pos, mine.slot, *work.w[(size_t)g], tmp[(size_t)g]);
            }));
            // the S temporary per-shard scopes form S temporary cluster scopes, never registered with the cluster
            std::unique_ptr<orr_cluster_scope[]> cs(new orr_cluster_scope[(size_t)S]);
            std::vector<const orr_cluster_scope *> ptrs((size_t)S);
            for (int32_t i = 0; i < S; ++i) {
                cs[(size_t)i].owner.store(c);
                for (int32_t g = 0; g < G; ++g) cs[(size_t)i].parts.push_back(&tmp[(size_t)g][(size_t)i]);
                ptrs[(size_t)i] = &cs[(size_t)i];
            }
            // ---- the search: C minus the exclusions, with no further limit
            SubBatch sb;
            BatchArgs cur;
            ORR_TRY(build_subset(lanes[0].lane, a, slice, sb, cur));           // (host-resident vectors: nothing of the lane is used)
            cur.topk = pool;
            cur.candidate_limit = std::max<int64_t>(1, all_rows);
            std::vector<int64_t> s_rows((size_t)S * pool, -1), s_keys((size_t)S * pool, -1);
            std::vector<double> s_scores((size_t)S * pool, 0.0);
            std::vector<int32_t> s_cnt((size_t)S, 0);
            cur.out_keys = s_keys.data();
            cluster_scope_begin(c, cur, s_rows.data(), s_scores.data(), s_cnt.data());
            if (S == 1) {
                ClusterScope one{true, 0, nullptr, nullptr};
                one.handle = ptrs[0];
                ORR_TRY(cluster_scope_on_lanes(c, fn, cur, one, lanes, true, false, s_rows.data(), s_scores.data(), s_cnt.data()));
            } else {
                std::vector<int32_t> qg((size_t)S);
                std::iota(qg.begin(), qg.end(), 0);
                ORR_TRY(cluster_grouped_on_lanes(c, fn, cur, S, ptrs.data(), qg.data(), lanes, s_rows.data(), s_scores.data(), s_cnt.data()));
            }
            memcpy(n_rows.data() + b0 * pool, s_rows.data(), sizeof(int64_t) * (size_t)S * pool);
            memcpy(n_keys.data() + b0 * pool, s_keys.data(), sizeof(int64_t) * (size_t)S * pool);
            memcpy(n_scores.data() + b0 * pool, s_scores.data(), sizeof(double) * (size_t)S * pool);
            memcpy(n_cnt.data() + b0, s_cnt.data(), sizeof(int32_t) * (size_t)S);
        }
        ids.swap(unfinished);
        r_rows.swap(n_rows); r_keys.swap(n_keys); r_scores.swap(n_scores); r_cnt.swap(n_cnt);
    }
    return ORR_OK;
}

}  // namespace

extern "C" {

int orr_cluster_keys_create(orr_cluster *c, int64_t n, const int64_t *row_ids, const int64_t *keys, orr_cluster_keys **out)
{
    static const char *fn = "orr_cluster_keys_create";
    if (!out) return fail(ORR_EINVAL, "%s: out is NULL", fn);
    if (n < 0) return fail(ORR_EINVAL, "%s: n is negative", fn);
    if (n > 0 && (!row_ids || !keys)) return fail(ORR_EINVAL, "%s: row_ids or keys is NULL with %lld entries", fn, (long long)n);
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (n > 0 && (is_device_pointer(row_ids) || is_device_pointer(keys))) return fail(ORR_EINVAL, "%s: row_ids and keys must be in host memory (every shard's device reads them)", fn);
    std::shared_lock<std::shared_mutex> lock(c->mu);   // like a search: beside the others; seal, compact, insert are exclusive
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    const int32_t G = (int32_t)c->shards.size();
    orr_cluster_keys *k = new (std::nothrow) orr_cluster_keys();
    if (!k) return fail(ORR_ENOMEM, "out of host memory");
    k->parts.assign((size_t)G, nullptr);
    const int r = for_each_shard(G, [&](int32_t g) -> int { return orr_keys_create(c->shards[(size_t)g], n, row_ids, keys, &k->parts[(size_t)g]); });
    if (r != ORR_OK) {
        const std::string keep = g_last_error;
        for (orr_keys *part : k->parts) orr_keys_destroy(part);
        delete k;
        g_last_error = keep;
        return r;
    }
    k->owner.store(c);
    { std::lock_guard<std::mutex> life(g_scope_life_mu); c->ckeys.push_back(k); }
    *out = k;
    return ORR_OK;
}

int orr_cluster_keys_set(orr_cluster_keys *k, int64_t n, const int64_t *row_ids, const int64_t *keys, int64_t *out_set)
{
    static const char *fn = "orr_cluster_keys_set";
    if (n < 0) return fail(ORR_EINVAL, "%s: n is negative", fn);
    if (n > 0 && (!row_ids || !keys)) return fail(ORR_EINVAL, "%s: row_ids or keys is NULL with %lld entries", fn, (long long)n);
    if (!k) return fail(ORR_EINVAL, "%s: null keys", fn);
    if (n > 0 && (is_device_pointer(row_ids) || is_device_pointer(keys))) return fail(ORR_EINVAL, "%s: row_ids and keys must be in host memory (every shard's device reads them)", fn);
    orr_cluster *c = nullptr;
    ORR_TRY(cluster_keys_owner(k, fn, &c));
    std::shared_lock<std::shared_mutex> lock(c->mu);
    const int32_t G = (int32_t)c->shards.size();
    std::vector<Lane> lanes;
    acquire_cluster_lanes(c, lanes);
    std::vector<std::unique_lock<std::shared_mutex>> held;     // every part exclusively, in ascending shard order
    held.reserve((size_t)G);
    for (int32_t g = 0; g < G; ++g) held.emplace_back(k->parts[(size_t)g]->mu);
    ORR_TRY(cluster_keys_owner(k, fn, &c));
    ORR_TRY(cluster_keys_parts_alive(c, k, fn));
    std::vector<int64_t> set((size_t)G, 0);
    const int r = for_each_shard(G, [&](int32_t g) -> int {
        orr_index *lane = lanes[(size_t)g].lane;
        std::lock_guard<std::mutex> l(lane->mu);
        return keys_set_held(lane, k->parts[(size_t)g], n, row_ids, keys, &set[(size_t)g]);
    });
    if (r != ORR_OK) {             // some shards may hold the edit and others not: never searched like that
        const std::string keep = g_last_error;
        held.clear();
        orphan_cluster_keys(k);
        g_last_error = keep;
        return r;
    }
    if (out_set) { *out_set = 0; for (int64_t s : set) *out_set += s; }
    return ORR_OK;
}

int orr_cluster_keys_get(orr_cluster_keys *k, int64_t n, const int64_t *row_ids, int64_t *out_keys)
{
    static const char *fn = "orr_cluster_keys_get";
    if (n < 0) return fail(ORR_EINVAL, "%s: n is negative", fn);
    if (n > 0 && (!row_ids || !out_keys)) return fail(ORR_EINVAL, "%s: row_ids or out_keys is NULL with %lld entries", fn, (long long)n);
    if (!k) return fail(ORR_EINVAL, "%s: null keys", fn);
    if (n > 0 && is_device_pointer(row_ids)) return fail(ORR_EINVAL, "%s: row_ids must be in host memory (every shard's device reads them)", fn);
    orr_cluster *c = nullptr;
    ORR_TRY(cluster_keys_owner(k, fn, &c));
    std::shared_lock<std::shared_mutex> lock(c->mu);
    const int32_t G = (int32_t)c->shards.size();
    std::vector<Lane> lanes;
    acquire_cluster_lanes(c, lanes);
    std::vector<std::shared_lock<std::shared_mutex>> held;     // every part shared, in ascending shard order
    held.reserve((size_t)G);
    for (int32_t g = 0; g < G; ++g) held.emplace_back(k->parts[(size_t)g]->mu);
    ORR_TRY(cluster_keys_owner(k, fn, &c));
    ORR_TRY(cluster_keys_parts_alive(c, k, fn));
    if (n == 0) return ORR_OK;
    std::vector<int64_t> got((size_t)G * (size_t)n, ORR_KEY_NONE);
    ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
        orr_index *lane = lanes[(size_t)g].lane;
        std::lock_guard<std::mutex> l(lane->mu);
        return keys_get_held(lane, k->parts[(size_t)g], c->shards[(size_t)g], n, row_ids, got.data() + (size_t)g * (size_t)n);
    }));
    for (int64_t i = 0; i < n; ++i) {                  // the lowest shard that has a key for the id
        out_keys[i] = ORR_KEY_NONE;
        for (int32_t g = 0; g < G && out_keys[i] == ORR_KEY_NONE; ++g) out_keys[i] = got[(size_t)g * (size_t)n + (size_t)i];
    }
    return ORR_OK;
}

int64_t orr_cluster_keys_rows(const orr_cluster_keys *k)
{
    if (!k || !k->owner.load()) return -1;
    int64_t n = 0;
    for (const orr_keys *part : k->parts) {
        const int64_t rows = orr_keys_rows(part);
        if (rows < 0) return -1;
        n += rows;
    }
    return n;
}

orr_keys *orr_cluster_keys_shard(orr_cluster_keys *k, int32_t shard)
{
    if (!k || shard < 0 || shard >= (int32_t)k->parts.size()) { (void)fail(ORR_EINVAL, "orr_cluster_keys_shard: no shard %d", shard); return nullptr; }
    return k->parts[(size_t)shard];
}

void orr_cluster_keys_destroy(orr_cluster_keys *k)
{
    if (!k) return;
    {   // (the cluster is not destroyed meanwhile; afterwards it no longer knows these keys)
        std::lock_guard<std::mutex> life(g_scope_life_mu);
        orr_cluster *c = k->owner.load();
        if (c) c->ckeys.erase(std::remove(c->ckeys.begin(), c->ckeys.end(), k), c->ckeys.end());
        k->owner.store(nullptr);
    }
    for (orr_keys *part : k->parts) orr_keys_destroy(part);        // each against its own shard's destroy, as a single column
    delete k;
}

int orr_cluster_scope_create_keys(orr_cluster *c, const orr_cluster_keys *k, int32_t n_keys, const int64_t *keys, orr_cluster_scope **out)
{
    static const char *fn = "orr_cluster_scope_create_keys";
    switch (per_key::first_invalid_scope_keys(!out, n_keys, !keys, !k)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out is NULL", fn);
    case 2: return fail(ORR_EINVAL, "%s: n_keys must be in 0 .. %d", fn, per_key::kMaxScopeKeys);
    case 3: return fail(ORR_EINVAL, "%s: keys is NULL with %d keys", fn, n_keys);
    default: return fail(ORR_EINVAL, "%s: null keys handle", fn);
    }
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    orr_cluster *own = k->owner.load();
    if (own && (own != c || k->parts.size() != c->shards.size())) return fail(ORR_EINVAL, "%s: the keys belong to another cluster", fn);
    ORR_TRY(cluster_keys_owner(k, fn, &own));
    if (n_keys > 0 && is_device_pointer(keys)) return fail(ORR_EINVAL, "%s: keys must be in host memory (every shard's device reads them)", fn);
    return make_cluster_scope(c, fn, out, [&](orr_index *sh, orr_scope **part) -> int {
        size_t g = 0;
        while (g < c->shards.size() && c->shards[g] != sh) ++g;
        if (g >= k->parts.size()) return fail(ORR_ESTATE, "%s: the keys do not cover this shard", fn);
        return orr_scope_create_keys(sh, k->parts[g], n_keys, keys, part);
    });
}

int orr_cluster_search_batch_per_key(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const uint8_t *terms_utf8, const uint32_t *term_off,
                                     const uint32_t *query_term_off, int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                                     const orr_cluster_scope *within, const orr_cluster_keys *keys, int32_t max_per_key, int32_t pool,
                                     int64_t *out_rows, double *out_scores, int64_t *out_keys, int32_t *out_counts, int32_t *out_rounds)
{
    static const char *fn = "orr_cluster_search_batch_per_key";
    switch (per_key::first_invalid(!out_rows || !out_scores || !out_keys || !out_counts, topk, pool, max_per_key, !keys)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out_rows, out_scores, out_keys and out_counts are required", fn);
    case 2: return fail(ORR_EINVAL, "%s: pool must be in 1 .. %d", fn, per_key::kMaxPool);
    case 3: return fail(ORR_EINVAL, "%s: topk %d exceeds the pool of %d", fn, topk, pool);
    case 4: return fail(ORR_EINVAL, "%s: max_per_key must be at least 1", fn);
    default: return fail(ORR_EINVAL, "%s: null keys", fn);
    }
    if (!c) return fail(ORR_EINVAL, "%s: null cluster", fn);
    if (B == 0) return ORR_OK;
    std::shared_lock<std::shared_mutex> lock(c->mu);   // from round 1 to the last round: no compaction or insertion moves a row in between
    if (!c->sealed) return fail(ORR_ESTATE, "%s: the cluster is not sealed", fn);
    orr_cluster *kown = keys->owner.load(), *sown = within ? within->owner.load() : nullptr;
    if (kown && (kown != c || keys->parts.size() != c->shards.size())) return fail(ORR_EINVAL, "%s: the keys belong to another cluster", fn);
    if (sown && (sown != c || within->parts.size() != c->shards.size())) return fail(ORR_EINVAL, "%s: the scope belongs to another cluster", fn);
    ORR_TRY(cluster_keys_owner(keys, fn, &kown));
    if (within) ORR_TRY(cluster_scope_owner(within, fn, &sown));
    if (dim > 0 && is_device_pointer(q_host)) return fail(ORR_EINVAL, "%s: the query vectors must be in host memory (every shard's device reads them)", fn);
    const BatchArgs a{B, dim, q_host, terms_utf8, term_off, query_term_off, now_ticks, candidate_limit, topk};
    ORR_TRY(check_batch(c->shards[0], a, fn));
    return cluster_per_key_run(c, fn, a, within, keys, max_per_key, pool, out_rows, out_scores, out_keys, out_counts, out_rounds);
}

}  // extern "C"

// ---- cluster key groups (orr_cluster_keys_groups, orr_cluster_keys_centroids, orr_cluster_scope_centroid) ----------------------
// The answers of the single-index calls on ONE index holding all the cluster's rows in the global candidate order, bit for bit.
// The pairs, the runs, the free blocks and every key that lies on one shard are the single index's helpers and records, run on
// every shard at once; what the cluster adds is orr_cluster_key_groups_plan.h's: a key's blocks of 256 are counted from its first
// member anywhere, so a spanning key's open block (P) and running sum (S) are carried from shard to shard in ascending order by
// keys_chain_step, through one pinned host buffer.

namespace {

// What a cluster key-groups call owns: every shard's work, chain records and state rows, and the pinned state of the slice in
// flight ([spanning keys][2][dim] fp64).  Each shard's buffers are released with its device bound.
struct ClusterKeyGroupsWork {
    std::vector<std::unique_ptr<KeyGroupsWork>> w;
    std::vector<DevBuf> chains, state;
    PinnedBuf pin;
    std::vector<int> device;
    explicit ClusterKeyGroupsWork(const orr_cluster *c) : chains(c->shards.size()), state(c->shards.size())
    {
        for (const orr_index *sh : c->shards) { w.emplace_back(new KeyGroupsWork()); device.push_back(sh->device); }
    }
    ~ClusterKeyGroupsWork()
    {
        for (size_t g = 0; g < w.size(); ++g) {
            (void)hipSetDevice(device[g]);
            w[g].reset();
            chains[g].release();
            state[g].release();
        }
        pin.release();
    }
};

// What the three calls hold: one lane per shard, all taken before any shard starts and in ascending shard order
// (acquire_in_order says why); behind them, on each shard, the scope part's lock, then the keys part's shared lock, as the single
// call takes them.  Then the handles looked at again: alive, of this cluster's shards, covering their shards' rows.
int cluster_key_groups_hold(orr_cluster *c, const char *fn, const orr_cluster_keys *k, const orr_cluster_scope *sc, std::vector<Lane> &lanes,
                            std::vector<std::shared_lock<std::shared_mutex>> &held)
{
    const size_t G = c->shards.size();
    std::vector<LanePool *> pools;
    std::vector<LanePool::Make> makes;
    for (orr_index *sh : c->shards) { pools.push_back(&sh->lanes); makes.push_back(lane_maker(sh)); }
    acquire_in_order(pools, makes, lanes);
    held.reserve(2 * G);
    for (size_t g = 0; g < G; ++g) {
        if (sc) held.emplace_back(sc->parts[g]->mu);
        if (k) held.emplace_back(k->parts[g]->mu);
    }
    orr_cluster *own = nullptr;
    if (k) {
        ORR_TRY(cluster_keys_owner(k, fn, &own));
        ORR_TRY(cluster_keys_parts_alive(c, k, fn));
    }
    if (sc) {
        ORR_TRY(cluster_scope_owner(sc, fn, &own));
        ORR_TRY(cluster_scope_parts_alive(c, sc, fn));
    }
    for (size_t g = 0; g < G; ++g) {
        const int64_t rows = lanes[g].lane->n_rows;
        if (k && k->parts[g]->n_rows != rows)
            return fail(ORR_ESTATE, "%s: the keys cover %lld rows of shard %d, the shard holds %lld", fn, (long long)k->parts[g]->n_rows, (int)g, (long long)rows);
        if (sc && sc->parts[g]->n_rows != rows)
            return fail(ORR_ESTATE, "%s: the scope covers %lld rows of shard %d, the shard holds %lld", fn, (long long)sc->parts[g]->n_rows, (int)g, (long long)rows);
    }
    return ORR_OK;
}

// Every lane's stream waited for and its launches folded into its shard's kernel statistics.
void cluster_key_groups_end(std::vector<Lane> &lanes)
{
    for (Lane &ln : lanes) {
        orr_index *lane = ln.lane;
        std::lock_guard<std::mutex> lock(lane->mu);
        if (bind_device(lane) != ORR_OK) continue;
        (void)hipStreamSynchronize(lane->stream);
        collect_events(lane);
    }
}

// The fp64 sums of the T keys of `table` (mode 1; the participating rows whose key it lists) or of the one group that is the scope
// (mode 2, T == 1) over all shards, slice by slice: emit(s0, ns, rows, total) receives per key of the slice where its dim sums lie
// (a spanning key's S in the pinned state, a home shard's row, a row of +0.0) with the keys' participating counts over the whole
// cluster.  The lanes and the handles' parts are held by the caller.
int cluster_key_groups_sums(orr_cluster *c, const char *fn, const orr_cluster_keys *k, const orr_cluster_scope *sc, int32_t mode,
                            const std::vector<int64_t> *table, int32_t T, int32_t dim, std::vector<Lane> &lanes, ClusterKeyGroupsWork &work,
                            const std::function<void(int32_t, int32_t, const double *const *, const int64_t *)> &emit)
{
    namespace ckg = cluster_key_groups;
    const int32_t G = (int32_t)c->shards.size();
    const size_t D = (size_t)dim;
    // ---- every shard at once: its pairs in candidate order, sorted by key, and its run table
    std::vector<std::vector<int64_t>> first((size_t)G, std::vector<int64_t>((size_t)T, 0)), count((size_t)G, std::vector<int64_t>((size_t)T, 0));
    ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
        orr_index *lane = lanes[(size_t)g].lane;
        if (lane->n_rows <= 0) return ORR_OK;
        std::lock_guard<std::mutex> lock(lane->mu);
        ORR_TRY(bind_device(lane));
        hipStream_t s = lane->stream;
        KeyGroupsWork &w = *work.w[(size_t)g];
        int64_t m = 0, runs = 0;
        ORR_TRY(key_groups_pairs(lane, k ? k->parts[(size_t)g] : nullptr, sc ? sc->parts[(size_t)g] : nullptr, mode, table, w, &m));
        if (mode == 2) { count[(size_t)g][0] = m; return ORR_OK; }
        ORR_TRY(key_groups_runs(lane, w, m, &runs));
        if (runs > T) return fail(ORR_EDEVICE, "%s: %lld runs of %d keys on shard %d", fn, (long long)runs, T, g);
        if (runs == 0) return ORR_OK;
        std::vector<uint64_t> rk((size_t)runs);
        std::vector<uint32_t> rl((size_t)runs);
        HIP_TRY(hipMemcpyAsync(rk.data(), w.run_key.p, sizeof(uint64_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(rl.data(), w.run_len.p, sizeof(uint32_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int64_t at = 0;
        for (int64_t i = 0; i < runs; ++i) {
            if (rk[(size_t)i] >= (uint64_t)T || at + (int64_t)rl[(size_t)i] > m) return fail(ORR_EDEVICE, "%s: a run outside the table on shard %d", fn, g);
            first[(size_t)g][(size_t)rk[(size_t)i]] = at;
            count[(size_t)g][(size_t)rk[(size_t)i]] = (int64_t)rl[(size_t)i];
            at += (int64_t)rl[(size_t)i];
        }
        return ORR_OK;
    }));
    // ---- the host: where each key's members on a shard lie among its members anywhere
    std::vector<std::vector<int64_t>> before((size_t)G, std::vector<int64_t>((size_t)T, 0));
    std::vector<int64_t> total((size_t)T, 0);
    for (int32_t t = 0; t < T; ++t)
        for (int32_t g = 0; g < G; ++g) { before[(size_t)g][(size_t)t] = total[(size_t)t]; total[(size_t)t] += count[(size_t)g][(size_t)t]; }
    // ---- the slices: the same keys of the call's table on every shard (the size changes no bit)
    const int32_t per_slice = key_groups::slice_keys(dim, lanes[0].lane->opt_key_groups_slice);
    const int32_t most = std::min(per_slice, T);
    const std::vector<double> zeros(D, 0.0);
    std::vector<const double *> rows((size_t)most);
    std::vector<int32_t> state((size_t)most), slot((size_t)most), home((size_t)most);
    std::vector<ckg::Records> rec((size_t)G);
    std::vector<double> sums((size_t)most * D);          // the home shards' rows of the slice in flight: shard g's from row local0[g] on
    std::vector<int64_t> local0((size_t)G + 1, 0);
    for (int32_t s0 = 0; s0 < T; s0 += per_slice) {
        const int32_t ns = std::min(per_slice, T - s0);
        // a key spans where some shard holds some but not all of its members; any other key with members has one home shard,
        // which keeps a row of sums for it
        int32_t n_span = 0;
        std::vector<int32_t> n_local((size_t)G, 0);
        for (int32_t j = 0; j < ns; ++j) {
            state[(size_t)j] = -1; slot[(size_t)j] = -1; home[(size_t)j] = -1;
            for (int32_t g = 0; g < G; ++g) {
                const int64_t n = count[(size_t)g][(size_t)(s0 + j)];
                if (ckg::spans(n, total[(size_t)(s0 + j)])) { state[(size_t)j] = n_span++; break; }
                if (n > 0) { home[(size_t)j] = g; slot[(size_t)j] = n_local[(size_t)g]++; break; }
            }
        }
        for (int32_t g = 0; g < G; ++g) local0[(size_t)g + 1] = local0[(size_t)g] + n_local[(size_t)g];
        const size_t state_bytes = sizeof(double) * 2 * D * (size_t)n_span;
        if (n_span) {
            ORR_TRY(work.pin.reserve(state_bytes));
            memset(work.pin.p, 0, state_bytes);
        }
        // ---- every shard at once: the free blocks, and the fold of the keys wholly there -- the single index's launches
        ORR_TRY(for_each_shard(G, [&](int32_t g) -> int {
            ckg::Records &r = rec[(size_t)g];
            r.clear();
            ckg::records_of(ns, count[(size_t)g].data() + s0, first[(size_t)g].data() + s0, before[(size_t)g].data() + s0, total.data() + s0, state.data(),
                            slot.data(), r);
            if (r.blocks.empty()) return ORR_OK;
            orr_index *lane = lanes[(size_t)g].lane;
            std::lock_guard<std::mutex> lock(lane->mu);
            ORR_TRY(bind_device(lane));
            hipStream_t s = lane->stream;
            KeyGroupsWork &w = *work.w[(size_t)g];
            ORR_TRY(key_groups_slice_launch(lane, w, n_local[(size_t)g], r.blocks, r.folds, r.n_parts));
            const size_t bytes = sizeof(double) * (size_t)n_local[(size_t)g] * D;
            if (bytes) HIP_TRY(hipMemcpyAsync(sums.data() + (size_t)local0[(size_t)g] * D, w.sums.p, bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            return ORR_OK;
        }));
        // ---- the chain: shards in ascending order, only where a spanning key of the slice has members
        for (int32_t g = 0; g < G && n_span; ++g) {
            const ckg::Records &r = rec[(size_t)g];
            if (r.chains.empty()) continue;             // (the carry passes over this shard)
            orr_index *lane = lanes[(size_t)g].lane;
            std::lock_guard<std::mutex> lock(lane->mu);
            ORR_TRY(bind_device(lane));
            hipStream_t s = lane->stream;
            KeyGroupsWork &w = *work.w[(size_t)g];
            uint32_t lo = r.chains[0].state, hi = lo;
            double head_rows = 0.0, part_rows = 0.0;
            for (const ckg::Chain &ch : r.chains) {
                lo = std::min(lo, ch.state); hi = std::max(hi, ch.state);
                head_rows += (double)ch.head_len;
                part_rows += (double)ch.n_close + 4.0;
                if (ch.state >= (uint32_t)n_span || ch.head_len >= (uint32_t)key_groups::kBlock ||
                    (size_t)ch.part0 + ch.n_close + (ckg::chain_open(ch.flags) == ckg::kOpenFree ? 1u : 0u) > (size_t)r.n_parts)
                    return fail(ORR_EDEVICE, "%s: a chain record outside its slice on shard %d", fn, g);
            }
            ORR_TRY(work.chains[(size_t)g].reserve(sizeof(ckg::Chain) * r.chains.size()));
            ORR_TRY(work.state[(size_t)g].reserve(state_bytes));
            // the state rows of the shard's spanning keys (one range of slots) go up, the step runs, the same rows come back
            const size_t off = sizeof(double) * 2 * D * (size_t)lo, len = sizeof(double) * 2 * D * (size_t)(hi - lo + 1);
            HIP_TRY(hipMemcpyAsync(work.chains[(size_t)g].p, r.chains.data(), sizeof(ckg::Chain) * r.chains.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(work.state[(size_t)g].as<char>() + off, work.pin.as<char>() + off, len, hipMemcpyHostToDevice, s));
            {
                Timed t(lane, "keys_chain_step", 4.0 * head_rows * (double)dim + 8.0 * part_rows * (double)dim);
                HIP_TRY(orr::launch_keys_chain_step(lane->d_emb, lane->n_rows, dim, w.pos, work.chains[(size_t)g].as<ckg::Chain>(), (int64_t)r.chains.size(),
                                                    w.parts.as<double>(), work.state[(size_t)g].as<double>(), s));
            }
            HIP_TRY(hipMemcpyAsync(work.pin.as<char>() + off, work.state[(size_t)g].as<char>() + off, len, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        // ---- the slice's rows: a spanning key's S, a home shard's row, +0.0 for a key without a participating member
        for (int32_t j = 0; j < ns; ++j) {
            if (state[(size_t)j] >= 0) rows[(size_t)j] = work.pin.as<double>() + (size_t)state[(size_t)j] * 2 * D;
            else if (home[(size_t)j] >= 0) rows[(size_t)j] = sums.data() + (size_t)(local0[(size_t)home[(size_t)j]] + slot[(size_t)j]) * D;
            else rows[(size_t)j] = zeros.data();
        }
        emit(s0, ns, rows.data(), total.data() + s0);
    }
    return ORR_OK;
}

}  // namespace

extern "C" {

int orr_cluster_keys_groups(orr_cluster_keys *k, const orr_cluster_scope *within, int64_t cap, int64_t *out_keys, int64_t *out_rows, int64_t *out_n,
                            int64_t *out_total)
{
    static const char *fn = "orr_cluster_keys_groups";
    switch (cluster_key_groups::first_invalid_groups(cap, !out_keys, !out_rows, !out_n, !out_total, !k)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: cap is negative", fn);
    case 2: return fail(ORR_EINVAL, "%s: out_n or out_total is NULL", fn);
    case 3: return fail(ORR_EINVAL, "%s: out_keys or out_rows is NULL with room for %lld keys", fn, (long long)cap);
    default: return fail(ORR_EINVAL, "%s: null keys", fn);
    }
    orr_cluster *c = nullptr, *sown = nullptr;
    ORR_TRY(cluster_keys_owner(k, fn, &c));
    if (within) ORR_TRY(cluster_scope_owner(within, fn, &sown));
    if (within && (sown != c || within->parts.size() != k->parts.size())) return fail(ORR_EINVAL, "%s: the scope belongs to another cluster", fn);
    std::shared_lock<std::shared_mutex> lock(c->mu);   // like a search: beside the others; seal, compact, insert are exclusive
    const int32_t G = (int32_t)c->shards.size();
    std::vector<Lane> lanes;
    std::vector<std::shared_lock<std::shared_mutex>> held;
    ORR_TRY(cluster_key_groups_hold(c, fn, k, within, lanes, held));
    ClusterKeyGroupsWork work(c);
    std::vector<std::vector<int64_t>> gk((size_t)G), gn((size_t)G);
    const int r = for_each_shard(G, [&](int32_t g) -> int {
        orr_index *lane = lanes[(size_t)g].lane;
        if (lane->n_rows <= 0) return ORR_OK;
        std::lock_guard<std::mutex> l(lane->mu);
        ORR_TRY(bind_device(lane));
        hipStream_t s = lane->stream;
        KeyGroupsWork &w = *work.w[(size_t)g];
        int64_t m = 0, runs = 0;
        ORR_TRY(key_groups_pairs(lane, k->parts[(size_t)g], within ? within->parts[(size_t)g] : nullptr, 0, nullptr, w, &m));
        ORR_TRY(key_groups_runs(lane, w, m, &runs));
        if (runs == 0) return ORR_OK;
        std::vector<uint32_t> len((size_t)runs);
        gk[(size_t)g].resize((size_t)runs);
        HIP_TRY(hipMemcpyAsync(gk[(size_t)g].data(), w.run_key.p, sizeof(uint64_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(len.data(), w.run_len.p, sizeof(uint32_t) * (size_t)runs, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        gn[(size_t)g].resize((size_t)runs);
        for (int64_t i = 0; i < runs; ++i) {
            gk[(size_t)g][(size_t)i] = key_groups::key_of_sort((uint64_t)gk[(size_t)g][(size_t)i]);
            gn[(size_t)g][(size_t)i] = (int64_t)len[(size_t)i];
        }
        return ORR_OK;
    });
    cluster_key_groups_end(lanes);
    if (r != ORR_OK) return r;
    std::vector<int64_t> mk, mn;
    const int64_t total = cluster_key_groups::merge_groups(gk, gn, cap, mk, mn);
    for (size_t i = 0; i < mk.size(); ++i) { out_keys[i] = mk[i]; out_rows[i] = mn[i]; }
    *out_total = total;
    *out_n = (int64_t)mk.size();
    return ORR_OK;
}

int orr_cluster_keys_centroids(orr_cluster_keys *k, const orr_cluster_scope *within, int32_t n_keys, const int64_t *keys, int32_t dim,
                               float *out_centroids, double *out_sums, int64_t *out_used)
{
    static const char *fn = "orr_cluster_keys_centroids";
    switch (cluster_key_groups::first_invalid_centroids(n_keys, !keys, !out_used, !k)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: n_keys must be in 0 .. %d", fn, key_groups::kMaxKeys);
    case 2: return fail(ORR_EINVAL, "%s: keys is NULL with %d keys", fn, n_keys);
    case 3: return fail(ORR_EINVAL, "%s: out_used is NULL with %d keys", fn, n_keys);
    default: return fail(ORR_EINVAL, "%s: null keys", fn);
    }
    orr_cluster *c = nullptr, *sown = nullptr;
    ORR_TRY(cluster_keys_owner(k, fn, &c));
    if (within) ORR_TRY(cluster_scope_owner(within, fn, &sown));
    if (within && (sown != c || within->parts.size() != k->parts.size())) return fail(ORR_EINVAL, "%s: the scope belongs to another cluster", fn);
    std::shared_lock<std::shared_mutex> lock(c->mu);
    std::vector<Lane> lanes;
    std::vector<std::shared_lock<std::shared_mutex>> held;
    ORR_TRY(cluster_key_groups_hold(c, fn, k, within, lanes, held));
    if (dim <= 0 || dim != lanes[0].lane->dim) return fail(ORR_EDIM, "%s: dim %d differs from the index dimension %d (and must be greater than 0)", fn, dim, lanes[0].lane->dim);
    if (n_keys == 0) return ORR_OK;
    if (is_device_pointer(keys)) return fail(ORR_EINVAL, "%s: keys must be in host memory (every shard's device reads them)", fn);
    // the sorted table of the distinct keys listed; the listed keys in the table's order (a key listed twice is answered twice)
    const std::vector<int64_t> table = per_key::member_table(keys, n_keys);
    const int32_t T = (int32_t)table.size();
    std::vector<int32_t> slot_of((size_t)n_keys), by_slot((size_t)n_keys);
    for (int32_t i = 0; i < n_keys; ++i) { slot_of[(size_t)i] = per_key::table_find(table.data(), T, keys[i]); by_slot[(size_t)i] = i; }
    std::stable_sort(by_slot.begin(), by_slot.end(), [&](int32_t a, int32_t b) { return slot_of[(size_t)a] < slot_of[(size_t)b]; });
    ClusterKeyGroupsWork work(c);
    size_t next = 0;                                   // of by_slot
    const int r = cluster_key_groups_sums(c, fn, k, within, 1, &table, T, dim, lanes, work, [&](int32_t s0, int32_t ns, const double *const *rows, const int64_t *total) {
        for (; next < by_slot.size() && slot_of[(size_t)by_slot[next]] < s0 + ns; ++next) {
            const int32_t i = by_slot[next], j = slot_of[(size_t)i] - s0;
            const double *S = rows[j];
            out_used[i] = total[j];
            if (out_sums) memcpy(out_sums + (size_t)i * (size_t)dim, S, sizeof(double) * (size_t)dim);
            if (out_centroids) key_groups::finish(S, total[j], dim, out_centroids + (size_t)i * (size_t)dim);
        }
    });
    cluster_key_groups_end(lanes);
    return r;
}

int orr_cluster_scope_centroid(orr_cluster_scope *sc, int32_t dim, float *out_centroid, double *out_sum, int64_t *out_used)
{
    static const char *fn = "orr_cluster_scope_centroid";
    switch (cluster_key_groups::first_invalid_scope_centroid(!out_used, !sc)) {
    case 0: break;
    case 1: return fail(ORR_EINVAL, "%s: out_used is NULL", fn);
    default: return fail(ORR_EINVAL, "%s: null scope", fn);
    }
    orr_cluster *c = nullptr;
    ORR_TRY(cluster_scope_owner(sc, fn, &c));
    std::shared_lock<std::shared_mutex> lock(c->mu);
    std::vector<Lane> lanes;
    std::vector<std::shared_lock<std::shared_mutex>> held;
    ORR_TRY(cluster_key_groups_hold(c, fn, nullptr, sc, lanes, held));
    if (dim <= 0 || dim != lanes[0].lane->dim) return fail(ORR_EDIM, "%s: dim %d differs from the index dimension %d (and must be greater than 0)", fn, dim, lanes[0].lane->dim);
    ClusterKeyGroupsWork work(c);
    std::vector<double> sum((size_t)dim, 0.0);
    int64_t used = 0;
    const int r = cluster_key_groups_sums(c, fn, nullptr, sc, 2, nullptr, 1, dim, lanes, work, [&](int32_t, int32_t, const double *const *rows, const int64_t *total) {
        memcpy(sum.data(), rows[0], sizeof(double) * (size_t)dim);
        used = total[0];
    });
    cluster_key_groups_end(lanes);
    if (r != ORR_OK) return r;
    *out_used = used;
    if (out_sum) memcpy(out_sum, sum.data(), sizeof(double) * (size_t)dim);
    if (out_centroid) key_groups::finish(sum.data(), used, dim, out_centroid);
    return ORR_OK;
}

}  // extern "C"
