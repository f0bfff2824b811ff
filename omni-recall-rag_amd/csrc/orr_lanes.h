// orr_lanes.h -- the search lanes of one index handle: all of their state, and the only code that touches it.
//
// Concurrent searches on ONE owning index each take a lane: the index itself (slot 0) or one of up to max_lanes - 1 internal
// views (own streams and workspaces, shared corpus and shadows), made when first needed.  Everything that changes what the lanes
// share or reads their counters (deletes, options, statistics, save, compact, destroy) runs under LanePool::Exclusive.
//
// Three rules:
//   1. Creation and Exclusive exclude each other.  acquire() neither takes nor makes a lane while the exclusive flag is set, and
//      Exclusive is not granted while a lane is held or being made.  So the set of lanes is fixed for as long as Exclusive is held.
//   2. Exclusive touches only its own flag: it never writes a busy mark, so it cannot hand out a lane somebody holds.
//   3. A caller that needs several lanes (one per shard of a cluster) takes them with acquire_in_order, on its own thread, in
//      ascending shard order.
//
// Host-only C++17, standard library only.  A lane is an opaque orr_index * here.
#pragma once

#include <cassert>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <mutex>
#include <vector>

struct orr_index;

class LanePool;

// What a search holds while it runs: one lane of a pool, given back by release() or the destructor.  A view handle the caller made
// itself (orr_index_view) is its own single lane and belongs to no pool: Lane::of(view).
struct Lane {
    orr_index *lane = nullptr;
    Lane() = default;
    static Lane of(orr_index *view) { Lane l; l.lane = view; return l; }
    Lane(const Lane &) = delete;
    Lane &operator=(const Lane &) = delete;
    Lane(Lane &&o) noexcept : lane(o.lane), pool_(o.pool_), slot_(o.slot_) { o.lane = nullptr; o.pool_ = nullptr; }
    ~Lane() { release(); }
    inline void release();

private:
    friend class LanePool;
    LanePool *pool_ = nullptr;
    size_t slot_ = 0;                  // 0: the owning index itself
};

class LanePool {
public:
    // Makes one more internal view of the owning index: 0 and the view on success.  An empty Make says that no lane may be made
    // at all (the index is not sealed yet); that is not a failure and leaves max_lanes alone.
    using Make = std::function<int(orr_index **)>;

    // Values the handle publishes beside its lanes: a lane or an exclusive operation writes them, and they are read without
    // waiting for searches (as a set: the pool's mutex covers them).
    struct Shared {
        int64_t dead_before = 0, dead_count = 0;       // copies of the index's dead_before / dead.size() for the cluster search
        uint32_t survivor_cap_hint = 0;                // a lane measured that the survivors' buffers must be at least this large
    };

    explicit LanePool(orr_index *self) { slots_.push_back(Slot{self, false, false}); }
    LanePool(const LanePool &) = delete;
    LanePool &operator=(const LanePool &) = delete;

    // A held lane: a free one, else a new one while fewer than max_lanes exist, else whichever is released first.  `make` runs
    // without the pool's mutex (it allocates workspaces and may wait for the search on slot 0).  When it fails there is no room
    // for another set of workspaces: max_lanes falls to the lanes there are and the caller waits for one of them.
    Lane acquire(const Make &make)
    {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            if (!exclusive_) {
                for (size_t i = 0; i < slots_.size(); ++i)
                    if (slots_[i].lane && !slots_[i].busy) { slots_[i].busy = true; return held(i); }
                if (make && lanes_or_coming() < max_lanes_) {
                    size_t i = 0;                               // a slot whose creation failed earlier, or a new one
                    while (i < slots_.size() && (slots_[i].lane || slots_[i].creating)) ++i;
                    if (i == slots_.size()) slots_.push_back(Slot{});
                    slots_[i].creating = true;
                    lk.unlock();
                    orr_index *v = nullptr;
                    const int r = make(&v);
                    lk.lock();
                    slots_[i].creating = false;
                    if (r == 0 && v) { slots_[i].lane = v; slots_[i].busy = true; return held(i); }
                    max_lanes_ = lanes_or_coming();             // the slot stays unusable (no lane in it)
                    cv_.notify_all();                           // (an Exclusive may have waited for this creation to end)
                    continue;                                   // a lane may have come free meanwhile
                }
            }
            cv_.wait(lk);
        }
    }

    // Waits until no lane is held and none is being made, and keeps searches out while it lives.
    class Exclusive {
    public:
        explicit Exclusive(LanePool *pool) : pool_(pool)       // (nullptr: a view handle, which has no pool -- nothing to wait for)
        {
            if (!pool_) return;
            std::unique_lock<std::mutex> lk(pool_->mu_);
            pool_->cv_.wait(lk, [this] {
                if (pool_->exclusive_) return false;
                for (const Slot &s : pool_->slots_) if (s.busy || s.creating) return false;
                return true;
            });
            pool_->exclusive_ = true;
        }
        ~Exclusive()
        {
            if (!pool_) return;
            { std::lock_guard<std::mutex> lk(pool_->mu_); pool_->exclusive_ = false; }
            pool_->cv_.notify_all();
        }
        Exclusive(const Exclusive &) = delete;
        Exclusive &operator=(const Exclusive &) = delete;

    private:
        LanePool *pool_;
    };

    // ---- under Exclusive only (the slots do not change then) ----
    template <class F> void for_each_lane(F &&fn)              // slot 0 and every view
    {
        assert(exclusive_);
        for (const Slot &s : slots_) if (s.lane) fn(s.lane);
    }
    std::vector<orr_index *> drain()                            // hands back the views (the caller destroys them); slot 0 alone stays
    {
        assert(exclusive_);
        std::lock_guard<std::mutex> lk(mu_);
        std::vector<orr_index *> views;
        for (size_t i = 1; i < slots_.size(); ++i) if (slots_[i].lane) views.push_back(slots_[i].lane);
        slots_.resize(1);
        return views;
    }
    void set_max_lanes(int n)                                   // (lanes that exist stay)
    {
        assert(exclusive_);
        std::lock_guard<std::mutex> lk(mu_);
        max_lanes_ = n > lanes_or_coming() ? n : lanes_or_coming();
    }

    // ---- any time ----
    Shared shared() { std::lock_guard<std::mutex> lk(mu_); return shared_; }
    template <class F> void update_shared(F &&fn) { std::lock_guard<std::mutex> lk(mu_); fn(shared_); }

private:
    friend struct Lane;
    struct Slot {
        orr_index *lane = nullptr;     // nullptr: being made, or unusable since its creation failed
        bool busy = false;             // a Lane holds it
        bool creating = false;         // reserved: its view is being made outside the mutex
    };
    Lane held(size_t i) { Lane l; l.lane = slots_[i].lane; l.pool_ = this; l.slot_ = i; return l; }
    int lanes_or_coming() const
    {
        int n = 0;
        for (const Slot &s : slots_) n += s.lane || s.creating;
        return n;
    }
    void release(size_t i)
    {
        { std::lock_guard<std::mutex> lk(mu_); slots_[i].busy = false; }
        cv_.notify_all();
    }

    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<Slot> slots_;          // [0] is the owning index
    int max_lanes_ = 4;
    bool exclusive_ = false;
    Shared shared_;
};

inline void Lane::release()
{
    if (pool_) pool_->release(slot_);
    pool_ = nullptr; lane = nullptr;
}

// One lane from each pool, taken on the calling thread in the order given; this is the only way to hold more than one lane.
// Every cluster search passes its shards in ascending shard index and a search on a single index holds one lane and waits for
// no other, so whoever waits for a lane of shard g holds lanes of shards below g only: no cycle of waiters can form.  Exclusive
// operations hold no lane while they wait, and the creation of a lane waits for nothing a lane holder waits for.
inline void acquire_in_order(const std::vector<LanePool *> &pools, const std::vector<LanePool::Make> &makes, std::vector<Lane> &out_lanes)
{
    out_lanes.clear();
    out_lanes.reserve(pools.size());
    for (size_t g = 0; g < pools.size(); ++g) out_lanes.push_back(pools[g]->acquire(makes[g]));
}
