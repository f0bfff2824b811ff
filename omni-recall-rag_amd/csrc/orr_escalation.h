// orr_escalation.h -- what happens to the queries of a batch whose top-k could not be certified: the rule, once.
//
// A pass leaves a certificate per query (finish_query).  The uncertified queries -- and only those -- are repeated as a compacted
// sub-batch through the next more exact pass.  The ladder, in the order decide() tries its rungs:
//   GrowBuffers  the same pass with larger survivors' buffers: when every uncertified query overflowed the buffers of some shard,
//                every shard kept survivors, and grown_survivor_cap accepts the measured counts on every shard that overflowed
//   Unfused      the batched pass without the fused epilogue: when some shard's pass was fused
//   Exact        the reference-arithmetic pass over all rows, same k': when some shard's pass went through the matrix cores
//   WiderK       k' x 4, at most the participating rows
//   Exhausted    k' already covers every participating row: nothing more exact exists, the results stand
// One index (orr_search_batch) is G = 1; a cluster passes one outcome per shard.  The driver is escalate() in orr_api.hip.
// A survivor_cap changes with GrowBuffers only: counts that ask for larger buffers while another rung is taken leave it alone.
//
// Three invariants of plan_pass (asserted at its end) let decide() read the flags of the pass instead of those of the batch:
//   1. fused() only without no_fuse       so "some pass was fused" already says that no_fuse is not set: Unfused is taken once
//   2. use_mfma only without force_exact  so "some pass used the matrix cores" says that force_exact is not set: Exact is taken once
//   3. two_stage() only when fused()      so no pass keeps survivors once no_fuse is set: GrowBuffers comes before Unfused only
//
// The ladder ends.  The driver sees to it that the repeat after GrowBuffers runs with buffers of at least the returned cap per
// query (the cap is kept as survivor_cap, and the repeat has no more queries, so select_fused halves it no further than before:
// queries x cap x 40 < queries x 2.25 worst x 40 < 2 GiB is what grown_survivor_cap checked).  Another GrowBuffers therefore
// needs a count above that cap, a cap is 8192 x 2^j, and counts of 2^19 and more are refused: at most 6 growths (8192 .. 2^18).
// Unfused and Exact set a flag that stays set: once each.  WiderK quadruples a k' >= 1 that was below n, and n <= 2^61 rows (so
// k' x 4 cannot wrap): at most 31 times.  That is kMaxRepeats = 6 + 1 + 1 + 31 repeats of a query at the most, in whatever
// order the rungs come; the driver fails with ORR_EDEVICE beyond it.
//
// repeat_only_if_grown is the one difference between the two callers that is kept (a later change may remove it: it alters which
// pass a query takes).  select_fused halves pass_cap below survivor_cap for large batches, so the cap the counts ask for may
// not exceed survivor_cap.  Without the flag (one index) the smaller sub-batch repeats the same pass all the same -- its
// buffers are halved less; with it (cluster) GrowBuffers needs a shard whose survivor_cap the decision raises, else the next rung.
//
// Host-only C++17, standard library and the plain C of omnirecall_hip.h (orr_search_stats); no HIP, no orr_index.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/omnirecall_hip.h"

namespace escalation {

constexpr int kMaxRepeats = 6 + 1 + 1 + 31;

// Passes whose workspace grows with (queries x rows) run over slices of the sub-batch, so that it stays below this.
constexpr size_t kPassWorkspaceBytes = (size_t)4 << 30;

// Queries per slice of a pass that keeps one number (8 bytes) per (query,row) -- the unfused and the exact one -- over n rows;
// 0: the nb queries go in one piece.
inline int32_t slice_width(int32_t nb, int64_t n, bool per_pair_pass)
{
    const size_t row_bytes = (size_t)std::max<int64_t>(n, 1) * 8;
    if (!per_pair_pass || nb <= 1 || (size_t)nb * row_bytes <= kPassWorkspaceBytes) return 0;
    return (int32_t)std::max<size_t>(1, kPassWorkspaceBytes / row_bytes);
}

// k' a search starts from: the asked k plus a margin, one selection list (sel_width = orr::kSelWidth) where that holds it.
inline int64_t initial_kprime(int32_t take, int64_t n, int32_t sel_width)
{
    const int64_t kprime = std::min<int64_t>(std::max<int64_t>(1, n), std::max<int64_t>((int64_t)take + 22, 32));
    return kprime > sel_width && take + 8 <= sel_width ? sel_width : kprime;
}

// The survivors' buffers a repeat of the screening pass needs when the buffers overflowed: `queries` queries, the worst of
// them kept `worst` survivors.  False where larger buffers are not the answer (too many survivors, or buffers of 2 GiB and
// more); else *cap = pass_cap doubled until it holds worst with an eighth to spare.
inline bool grown_survivor_cap(uint32_t pass_cap, uint32_t worst, int64_t n, size_t queries, uint32_t *cap)
{
    if (worst >= (1u << 19) || (int64_t)worst * 2 >= n || queries * (size_t)worst * 96 >= ((size_t)2 << 30)) return false;
    *cap = pass_cap;
    while (*cap < worst + worst / 8) *cap *= 2;
    return true;
}

// What one shard's pass over nb queries left behind (a copy: the lane that ran it may serve another search meanwhile).
struct ShardOutcome {
    bool two_stage = false, fused = false, use_mfma = false;   // PassPlan::two_stage(), fused(), use_mfma
    uint32_t pass_cap = 0;               // entries per query of the survivors' buffers the pass used
    uint32_t survivor_cap = 0;           // what the lane keeps for its next pass (>= pass_cap)
    int64_t n = 0;                       // participating rows of the shard
    int64_t pass_mode = 0;               // orr_search_stats.pass_mode after the pass
    std::vector<uint32_t> survivors;     // (query,row) pairs the screen kept, per query; empty: the pass kept none

    bool kept(size_t nb) const { return two_stage && survivors.size() == nb; }
    bool overflowed(size_t i) const { return survivors[i] > pass_cap; }
};

// The survivors' counters of `s` after one shard's pass over nb queries.
inline void account_survivors(orr_search_stats &s, const ShardOutcome &o, size_t nb)
{
    if (!o.kept(nb)) return;
    for (size_t i = 0; i < nb; ++i) {
        s.survivors_total += o.survivors[i];
        s.survivors_max = std::max<int64_t>(s.survivors_max, o.survivors[i]);
        s.overflowed_queries += o.overflowed(i);
    }
    s.survivor_samples += (int64_t)nb;
    s.survivor_capacity = std::max<int64_t>(s.survivor_capacity, o.survivor_cap);
}

// `lane`'s counters added to `into` (the lanes of one handle): sums, the maxima of survivors_max and survivor_capacity, the
// pass_mode of the first that has one.  vocab_tokens (the shared corpus) and reserved are no counters of a lane: left alone.
inline void add_search_stats(orr_search_stats &into, const orr_search_stats &lane)
{
    into.searches += lane.searches; into.queries += lane.queries; into.passes += lane.passes; into.requeried += lane.requeried;
    into.overflowed_queries += lane.overflowed_queries; into.buffer_growths += lane.buffer_growths;
    into.exact_pass_queries += lane.exact_pass_queries; into.survivors_total += lane.survivors_total;
    into.survivor_samples += lane.survivor_samples; into.survivors_max = std::max(into.survivors_max, lane.survivors_max);
    into.survivor_capacity = std::max(into.survivor_capacity, lane.survivor_capacity);
    into.kw_hits_total += lane.kw_hits_total; into.kw_passes += lane.kw_passes;
    if (into.pass_mode == 0) into.pass_mode = lane.pass_mode;
}

enum class Step { Done, GrowBuffers, Unfused, Exact, WiderK, Exhausted };

struct Decision {
    Step step = Step::Done;
    std::vector<int32_t> again;          // the queries to repeat (positions in the pass's sub-batch, ascending); none when the ladder ends
    std::vector<uint32_t> new_cap;       // GrowBuffers: per shard, the survivor_cap its counts ask for (0: it did not overflow)
    int64_t kprime = 0;                  // k' of the repeat
};

// The next step after one pass of G >= 1 shards over the queries certified[0 .. nb): shards[g] is shard g's outcome, n_total
// the participating rows of all shards, no_fuse / force_exact / kprime what the pass ran with.
inline Decision decide(const std::vector<ShardOutcome> &shards, const std::vector<uint8_t> &certified, bool no_fuse, bool force_exact,
                       int64_t kprime, int64_t n_total, bool repeat_only_if_grown)
{
    const size_t nb = certified.size();
    Decision d;
    d.kprime = kprime;
    for (size_t i = 0; i < nb; ++i) if (!certified[i]) d.again.push_back((int32_t)i);
    if (d.again.empty()) return d;

    // larger buffers answer when overflow is the whole reason: every uncertified query overflowed somewhere ...
    bool only_overflow = true, raised = false, any_fused = false, any_mfma = false;
    for (const ShardOutcome &o : shards) {
        only_overflow = only_overflow && o.kept(nb);
        any_fused = any_fused || o.fused;
        any_mfma = any_mfma || o.use_mfma;
    }
    for (size_t a = 0; a < d.again.size() && only_overflow; ++a) {
        bool over = false;
        for (const ShardOutcome &o : shards) over = over || o.overflowed((size_t)d.again[a]);
        only_overflow = over;
    }
    // ... and every shard that overflowed can buffer what its worst uncertified query kept
    d.new_cap.assign(shards.size(), 0);
    for (size_t g = 0; g < shards.size() && only_overflow; ++g) {
        const ShardOutcome &o = shards[g];
        uint32_t worst = 0;
        for (int32_t i : d.again) if (o.overflowed((size_t)i)) worst = std::max(worst, o.survivors[(size_t)i]);
        if (worst == 0) continue;
        only_overflow = grown_survivor_cap(o.pass_cap, worst, o.n, d.again.size(), &d.new_cap[g]);
        raised = raised || (only_overflow && d.new_cap[g] > o.survivor_cap);
    }
    if (only_overflow && (raised || !repeat_only_if_grown)) {
        d.step = Step::GrowBuffers;
        return d;
    }
    d.new_cap.clear();
    if (any_fused && !no_fuse) {
        d.step = Step::Unfused;          // a tie at the cut, or an overflow too large to buffer
    } else if (any_mfma && !force_exact) {
        d.step = Step::Exact;
    } else if (kprime >= n_total) {
        d.step = Step::Exhausted;
        d.again.clear();
    } else {
        d.step = Step::WiderK;
        d.kprime = std::min<int64_t>(n_total, kprime * 4);
    }
    return d;
}

}  // namespace escalation
