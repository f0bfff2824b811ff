// orr_lanes_selftest -- the lane pool's protocol (../orr_lanes.h) on the CPU: no HIP, no GPU.
//
//   orr_lanes_selftest <scenario>      exit status 0: the scenario held; 1: a check failed; 2: usage; 3: the deadline passed
//
// A lane is an empty struct here, and "searching" on one is counting its holders.  The pool's own waits have no limit, so a
// watchdog ends the process when a scenario has not finished within its deadline: a broken protocol fails, it does not hang.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

struct orr_index {};
#include "../orr_lanes.h"

namespace {

using namespace std::chrono_literals;
constexpr auto kDeadline = 60s;       // per scenario (they take well under a second; a loaded machine or ThreadSanitizer gets room)
constexpr auto kSettle = 150ms;       // how long "does not happen" is watched

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); fflush(stderr); std::_Exit(1); } \
    } while (0)

// waits (with a limit) until a flag another thread sets is up
void await(const std::atomic<bool> &flag)
{
    const auto end = std::chrono::steady_clock::now() + kDeadline / 2;
    while (!flag.load()) {
        CHECK(std::chrono::steady_clock::now() < end);
        std::this_thread::sleep_for(1ms);
    }
}

// who holds what: every holder of a lane enters and leaves here
struct Ledger {
    std::mutex mu;
    std::map<orr_index *, int> holders;
    int held = 0, max_held = 0;
    void enter(orr_index *l)
    {
        std::lock_guard<std::mutex> lk(mu);
        CHECK(l != nullptr);
        CHECK(++holders[l] == 1);                      // no slot has two holders
        if (++held > max_held) max_held = held;
    }
    void leave(orr_index *l)
    {
        std::lock_guard<std::mutex> lk(mu);
        CHECK(--holders[l] == 0);
        --held;
    }
    int now() { std::lock_guard<std::mutex> lk(mu); return held; }
};

struct Fixture {
    orr_index self;
    LanePool pool{&self};
    Ledger ledger;
    std::atomic<int> makes{0};
    std::mutex made_mu;
    std::set<orr_index *> made;
    LanePool::Make make = [this](orr_index **out) {
        ++makes;
        *out = new orr_index();
        std::lock_guard<std::mutex> lk(made_mu);
        made.insert(*out);
        return 0;
    };
    void set_max_lanes(int n) { LanePool::Exclusive all(&pool); pool.set_max_lanes(n); }
    void search(const LanePool::Make &mk)
    {
        Lane ln = pool.acquire(mk);
        ledger.enter(ln.lane);
        std::this_thread::yield();
        ledger.leave(ln.lane);
    }
    int count_lanes()
    {
        LanePool::Exclusive all(&pool);
        int n = 0;
        pool.for_each_lane([&](orr_index *) { ++n; });
        return n;
    }
};

void join_all(std::vector<std::thread> &threads) { for (std::thread &t : threads) t.join(); }

// 16 threads, 4 lanes: never more than 4 held, no lane with two holders, at most 3 views made, every thread finishes
void more_threads_than_lanes()
{
    Fixture f;
    f.set_max_lanes(4);
    std::vector<std::thread> threads;
    for (int t = 0; t < 16; ++t) threads.emplace_back([&] { for (int i = 0; i < 2000; ++i) f.search(f.make); });
    join_all(threads);
    CHECK(f.ledger.max_held <= 4);
    CHECK(f.makes.load() <= 3);
    CHECK(f.count_lanes() == 1 + f.makes.load());
}

// Exclusive is not granted while a lane is being made, and no lane is made while Exclusive is held
void exclusive_against_creation()
{
    Fixture f;
    std::atomic<bool> a_in_make{false}, make_may_return{false}, a_holds{false}, a_may_release{false}, a_released{false};
    std::atomic<bool> b_granted{false}, b_may_release{false}, c_granted{false};
    Lane self = f.pool.acquire(f.make);                // slot 0 is taken: A has to make a lane
    CHECK(f.makes.load() == 0);
    std::thread a([&] {
        Lane ln = f.pool.acquire([&](orr_index **out) {
            a_in_make = true;
            await(make_may_return);
            return f.make(out);
        });
        f.ledger.enter(ln.lane);
        a_holds = true;
        await(a_may_release);
        f.ledger.leave(ln.lane);
        a_released = true;
        ln.release();
    });
    await(a_in_make);
    self.release();                                    // only the lane being made stands between B and Exclusive now
    std::thread b([&] {
        LanePool::Exclusive all(&f.pool);
        CHECK(a_released.load());                      // not before A's make has returned and A has let go
        CHECK(f.ledger.now() == 0);
        b_granted = true;
        await(b_may_release);
    });
    std::this_thread::sleep_for(kSettle);
    CHECK(!b_granted.load());                          // A is inside make
    make_may_return = true;
    await(a_holds);
    std::this_thread::sleep_for(kSettle);
    CHECK(!b_granted.load());                          // A holds the new lane
    a_may_release = true;
    await(b_granted);
    std::thread c([&] {                                // arrives while B holds Exclusive: waits, and makes nothing
        Lane ln = f.pool.acquire(f.make);
        f.ledger.enter(ln.lane);
        c_granted = true;
        f.ledger.leave(ln.lane);
    });
    std::this_thread::sleep_for(kSettle);
    CHECK(!c_granted.load());
    CHECK(f.makes.load() == 1);
    b_may_release = true;
    await(c_granted);
    a.join(); b.join(); c.join();
    CHECK(f.makes.load() == 1);                        // C took a free lane
    CHECK(f.count_lanes() == 2);
}

// one thread takes and drops Exclusive (and drains, so that lanes are made again right before the next round) while 15 search
void exclusive_against_searches()
{
    Fixture f;
    std::atomic<bool> stop{false};
    std::vector<std::thread> threads;
    for (int t = 0; t < 15; ++t) threads.emplace_back([&] { while (!stop.load()) f.search(f.make); });
    size_t drained = 0;
    for (int round = 0; round < 100; ++round) {
        {
            LanePool::Exclusive all(&f.pool);
            for (int i = 0; i < 20; ++i) { CHECK(f.ledger.now() == 0); std::this_thread::yield(); }
            int lanes = 0;
            f.pool.for_each_lane([&](orr_index *) { ++lanes; });
            CHECK(lanes >= 1 && lanes <= 4);
            if (round % 2) drained += f.pool.drain().size();     // (the lanes stay alive in f.made: a stale holder would show in the ledger)
        }
        std::this_thread::sleep_for(200us);
    }
    stop = true;
    join_all(threads);
    CHECK(f.ledger.max_held <= 4);
    CHECK(drained + (size_t)f.count_lanes() - 1 == (size_t)f.makes.load());
}

// make fails: max_lanes falls to the lanes there are, the failed slot is never handed out, waiters go on with what exists
void make_fails()
{
    Fixture f;
    std::atomic<int> calls{0};
    LanePool::Make flaky = [&](orr_index **out) {
        std::this_thread::sleep_for(1ms);
        if (calls.fetch_add(1) == 0) return f.make(out);
        *out = nullptr;
        return 1;
    };
    std::vector<std::thread> threads;
    for (int t = 0; t < 8; ++t) threads.emplace_back([&] { for (int i = 0; i < 1000; ++i) f.search(flaky); });
    join_all(threads);
    CHECK(f.makes.load() == 1);
    CHECK(f.ledger.max_held <= 2);
    CHECK(calls.load() <= 4);                          // every failure lowers max_lanes (4 at the start) by at least one
    CHECK(f.count_lanes() == 2);
    for (const auto &h : f.ledger.holders) CHECK(h.first == &f.self || f.made.count(h.first));
}

// drain hands back exactly the views made; afterwards the pool grows again up to max_lanes
void drain_and_regrowth()
{
    Fixture f;
    {
        std::vector<Lane> all4;
        for (int i = 0; i < 4; ++i) all4.push_back(f.pool.acquire(f.make));
        CHECK(all4[0].lane == &f.self);
        CHECK(f.makes.load() == 3);
    }
    const std::set<orr_index *> first = f.made;
    {
        LanePool::Exclusive all(&f.pool);
        const std::vector<orr_index *> views = f.pool.drain();
        CHECK(std::set<orr_index *>(views.begin(), views.end()) == first && views.size() == 3);
        int lanes = 0;
        f.pool.for_each_lane([&](orr_index *l) { CHECK(l == &f.self); ++lanes; });
        CHECK(lanes == 1);
        CHECK(f.pool.drain().empty());
    }
    std::vector<Lane> all4;
    for (int i = 0; i < 4; ++i) {
        all4.push_back(f.pool.acquire(f.make));
        CHECK(all4.back().lane == &f.self || !first.count(all4.back().lane));
    }
    CHECK(f.makes.load() == 6);
    std::atomic<bool> fifth{false};
    std::thread t([&] { Lane ln = f.pool.acquire(f.make); fifth = true; });
    std::this_thread::sleep_for(kSettle);
    CHECK(!fifth.load());                              // four lanes, four holders
    all4.pop_back();
    await(fifth);
    t.join();
    CHECK(f.makes.load() == 6);
}

// 3 pools of one lane each, 6 threads that each take all three in ascending order: all finish
void ordered_acquisition()
{
    Fixture f[3];
    LanePool::Make fails = [](orr_index **out) { *out = nullptr; return 1; };
    std::vector<LanePool *> pools;
    for (Fixture &x : f) pools.push_back(&x.pool);
    const std::vector<LanePool::Make> makes(3, fails);
    std::vector<std::thread> threads;
    for (int t = 0; t < 6; ++t)
        threads.emplace_back([&] {
            for (int i = 0; i < 500; ++i) {
                std::vector<Lane> lanes;
                acquire_in_order(pools, makes, lanes);
                CHECK(lanes.size() == 3);
                for (int g = 0; g < 3; ++g) { CHECK(lanes[(size_t)g].lane == &f[g].self); f[g].ledger.enter(lanes[(size_t)g].lane); }
                std::this_thread::yield();
                for (int g = 0; g < 3; ++g) f[g].ledger.leave(lanes[(size_t)g].lane);
                lanes.clear();
            }
        });
    join_all(threads);
    for (Fixture &x : f) { CHECK(x.ledger.max_held == 1); CHECK(x.count_lanes() == 1); }
}

const struct { const char *name; void (*run)(); } kScenarios[] = {
    {"more_threads_than_lanes", more_threads_than_lanes},
    {"exclusive_against_creation", exclusive_against_creation},
    {"exclusive_against_searches", exclusive_against_searches},
    {"make_fails", make_fails},
    {"drain_and_regrowth", drain_and_regrowth},
    {"ordered_acquisition", ordered_acquisition},
};

}  // namespace

int main(int argc, char **argv)
{
    for (const auto &s : kScenarios) {
        if (argc != 2 || strcmp(argv[1], s.name) != 0) continue;
        std::thread([] {
            std::this_thread::sleep_for(kDeadline);
            fprintf(stderr, "deadline passed: threads are still waiting\n");
            fflush(stderr);
            std::_Exit(3);
        }).detach();
        s.run();
        printf("%s ok\n", s.name);
        fflush(stdout);
        std::_Exit(0);                                 // (the watchdog is still asleep)
    }
    fprintf(stderr, "usage: orr_lanes_selftest <scenario>, one of:\n");
    for (const auto &s : kScenarios) fprintf(stderr, "  %s\n", s.name);
    return 2;
}
