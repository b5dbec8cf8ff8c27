// The stash of the one-shot calls (csrc/stash.h) on its own, with fake contexts: every transition on one thread, then 8 threads that
// run the four call shapes of csrc/oneshot.hip against one stash.  Built with -fsanitize=address,undefined and again with
// -fsanitize=thread by tests/test_stash_host.py; prints "ok" and exits 0, or says which check failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "stash.h"

using namespace mvs;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

// a mutex that knows whether the calling thread holds it
struct OwnedMutex {
    std::mutex m; std::atomic<std::thread::id> owner{std::thread::id()};
    void lock() { m.lock(); owner.store(std::this_thread::get_id()); }
    void unlock() { owner.store(std::thread::id()); m.unlock(); }
    bool held_by_me() const { return owner.load() == std::this_thread::get_id(); }
    bool try_lock() { if (held_by_me() || !m.try_lock()) return false; owner.store(std::this_thread::get_id()); return true; }
};

struct Fake { std::atomic<int> owned{0}, destroyed{0}; };
using TestStash = Stash<Fake, OwnedMutex>;
namespace mvs { struct StashTestAccess { static OwnedMutex& mutex(TestStash& s) { return s.m_; } }; }

// Fakes are never freed while the program runs: a second destroy of one finds its flag, not freed memory.
// One word holds {contexts held by threads, live contexts}: the two are read as one snapshot.  A thread holds a context from the moment
// a take_* (from before the call) or make() gave it one until its park_* or destroy has returned (the context a park_* displaces is the parking thread's to
// destroy: it counts as held by it), so at every instant live <= held + 2, the two slots.
constexpr uint64_t HELD = 1ull << 32;
static std::vector<Fake> g_pool;
static std::atomic<uint32_t> g_made{0}, g_destroyed{0};
static std::atomic<uint64_t> g_held_live{0};
static TestStash* g_stash = nullptr;
static bool g_single_thread = true;

static void check_bound() { const uint64_t v = g_held_live.load(); CHECK((v & 0xFFFFFFFFull) <= (v >> 32) + 2); }
static Fake* make() {
    const uint32_t k = g_made.fetch_add(1);
    CHECK(k < g_pool.size());
    g_held_live.fetch_add(HELD + 1);
    Fake* f = &g_pool[k];
    CHECK(f->owned.exchange(1) == 0);
    return f;
}
static void destroy(Fake* f) {
    CHECK(f != nullptr);
    CHECK(!StashTestAccess::mutex(*g_stash).held_by_me());                               // never with the stash's mutex held
    if (g_single_thread) { CHECK(StashTestAccess::mutex(*g_stash).try_lock()); StashTestAccess::mutex(*g_stash).unlock(); }
    CHECK(f->destroyed.exchange(1) == 0);                                // exactly once
    g_destroyed.fetch_add(1);
    g_held_live.fetch_sub(1);
}
// a context a take_* handed out belongs to this thread alone; one about to be parked or destroyed no longer does
// (counted as held from before the take_*: once the context has left its slot another thread may fill that slot)
template <class Take>
static Fake* own(Take&& take) {
    g_held_live.fetch_add(HELD);
    Fake* f = take();
    if (f) { CHECK(f->destroyed.load() == 0); CHECK(f->owned.exchange(1) == 0); } else g_held_live.fetch_sub(HELD);
    check_bound();
    return f;
}
static Fake* disown(Fake* f) { CHECK(f->owned.exchange(0) == 1); return f; }
static void released() { check_bound(); g_held_live.fetch_sub(HELD); }   // the park_* or destroy of a held context has returned
static void give_table(TestStash& S, Fake* c, uint64_t fp, const TableShape& shape) { S.park_table(disown(c), fp, shape); released(); }
static void give_spare(TestStash& S, Fake* c) { S.park_spare(disown(c)); released(); }
static void drop(Fake* c) { destroy(disown(c)); released(); }
static uint32_t live() { return g_made.load() - g_destroyed.load(); }

static void single_threaded() {
    TestStash S(destroy); g_stash = &S;
    const TableShape A{100, 7, 555};
    CHECK(S.take_working() == nullptr && S.take_spare() == nullptr && S.take_table(1, A) == nullptr && !S.shape_matches(A));
    S.park_spare(nullptr);   // no-op
    CHECK(S.take_spare() == nullptr);

    // take_table: fingerprint and all three shape fields; shape_matches agrees on the shape
    Fake* a = make();
    give_table(S, a, 0xABCDull, A);
    const TableShape wrong[3] = {{101, 7, 555}, {100, 8, 555}, {100, 7, 556}};
    for (const TableShape& w : wrong) { CHECK(!S.shape_matches(w)); CHECK(S.take_table(0xABCDull, w) == nullptr); }
    CHECK(S.shape_matches(A));
    CHECK(S.take_table(0xABCEull, A) == nullptr);   // right shape, another table
    CHECK(S.shape_matches(A));
    CHECK(own([&] { return S.take_table(0xABCDull, A); }) == a);
    CHECK(!S.shape_matches(A) && S.take_table(0xABCDull, A) == nullptr);   // handed out: in no slot
    CHECK(S.take_working() == nullptr);

    // park table A, then B: A is destroyed, once
    const TableShape B{200, 9, 777};
    Fake* b = make();
    give_table(S, a, 1, A);
    CHECK(live() == 2);
    give_table(S, b, 2, B);
    CHECK(a->destroyed.load() == 1 && b->destroyed.load() == 0 && live() == 1);
    CHECK(S.take_table(1, A) == nullptr && !S.shape_matches(A) && S.shape_matches(B));

    // take_working prefers the spare and leaves the parked table alone ...
    Fake* s = make();
    give_spare(S, s);
    CHECK(own([&] { return S.take_working(); }) == s);
    CHECK(S.shape_matches(B));
    // ... and without a spare takes the parked table's context, whose fingerprint is forgotten
    CHECK(own([&] { return S.take_working(); }) == b);
    CHECK(!S.shape_matches(B) && S.take_table(2, B) == nullptr && S.take_working() == nullptr);
    give_spare(S, b);
    CHECK(S.take_table(2, B) == nullptr && !S.shape_matches(B));   // a spare is no table
    // take_spare never hands out the parked table's context
    CHECK(own([&] { return S.take_spare(); }) == b);
    give_table(S, b, 2, B);
    CHECK(S.take_spare() == nullptr && S.shape_matches(B));

    // park_spare over a spare destroys the old one
    Fake* s2 = make();
    give_spare(S, s);
    give_spare(S, s2);
    CHECK(s->destroyed.load() == 1 && s2->destroyed.load() == 0 && live() == 2);

    // release_all empties both slots, twice
    S.release_all();
    CHECK(live() == 0 && b->destroyed.load() == 1 && s2->destroyed.load() == 1);
    CHECK(S.take_working() == nullptr && S.take_spare() == nullptr && S.take_table(2, B) == nullptr && !S.shape_matches(B));
    S.release_all();
    CHECK(live() == 0 && g_made.load() == g_destroyed.load());
    CHECK(g_held_live.load() == 0);
    g_stash = nullptr;
}

// ---- 8 threads, the call shapes of oneshot.hip ----
constexpr int THREADS = 8, ROUNDS = 4000;
static uint32_t next(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

static void worker(TestStash* S, int id) {
    uint64_t rng = 0x9E3779B97F4A7C15ull * (uint64_t)(id + 1);
    // a few tables that different threads agree on: fingerprint k has shape {k, k, k}
    auto table = [&](uint32_t r) { return 1 + r % 3; };
    for (int round = 0; round < ROUNDS; ++round) {
        const uint32_t r = next(rng), k = table(next(rng));
        const TableShape shape{k, k, (uint64_t)k};
        switch (r % 4) {
        case 0: {   // data costs succeed: the table is parked
            Fake* c = own([&] { return S->take_working(); }); if (!c) c = make();
            check_bound();
            give_table(*S, c, k, shape);
            break; }
        case 1: {   // data costs fail: the working context is destroyed, whatever it was parked with
            Fake* c = own([&] { return S->take_working(); }); if (!c) c = make();
            check_bound();
            drop(c);
            break; }
        case 2: {   // view selection: the parked table if it is the caller's, else the spare, else a new context
            Fake* c = S->shape_matches(shape) ? own([&] { return S->take_table(k, shape); }) : nullptr;
            if (!c) c = own([&] { return S->take_spare(); });
            if (!c) c = make();
            check_bound();
            if (next(rng) % 8) give_spare(*S, c); else drop(c);   // solved, or failed
            break; }
        default: {  // the cached call: only the parked table
            Fake* c = own([&] { return S->take_table(k, shape); });
            check_bound();
            if (c) give_spare(*S, c);
            break; }
        }
    }
}

static void threaded() {
    TestStash S(destroy); g_stash = &S; g_single_thread = false;
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t) th.emplace_back(worker, &S, t);
    for (auto& x : th) x.join();
    CHECK(g_held_live.load() >> 32 == 0);
    CHECK(live() <= 2);
    S.release_all();
    CHECK(g_made.load() == g_destroyed.load() && g_held_live.load() == 0);
    CHECK(S.take_working() == nullptr);
    g_stash = nullptr;
}

int main() {
    g_pool = std::vector<Fake>((size_t)THREADS * ROUNDS + 64);
    single_threaded();
    threaded();
    printf("ok\n");
    return 0;
}
