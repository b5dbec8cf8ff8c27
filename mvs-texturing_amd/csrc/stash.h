// stash.h -- the two contexts the one-shot calls keep between them (plain host C++, no HIP; tests/cpp/test_stash.cpp drives it with a
// fake context).
// texrecon calls tex::calculate_data_costs and tex::view_selection back to back with the same DataCosts (texrecon.cpp:100,121).
// mvs_data_costs therefore parks its context -- table resident -- together with a fingerprint of the table it handed out;
// mvs_view_selection fingerprints the table it is given and, if it is the same one, solves on the parked context: no context set-up, no
// 0.5 GB upload at BASELINE config 3.  A table the caller changed, loaded from a file or computed elsewhere has another fingerprint and
// is uploaded as before.  The second slot, the spare, is a context without a table to keep: its stream, buffers and instantiated graph
// serve the next one-shot call.  MVS_KEEP_TABLE=0 switches the stash off (the callers ask stash_enabled()); mvs_release_cached() empties it.
//
// Any thread may call any operation.  Invariants:
//   * a context is in at most one slot;
//   * a context handed out by a take_* is in no slot: it belongs to the caller, who parks it again or destroys it;
//   * a context displaced by a park_* (or taken out by release_all) is destroyed exactly once, and never with the mutex held -- a
//     context parked earlier by another thread, or by a call whose view selection never came, does not orphan a scene on the device;
//   * after release_all() nothing is parked.
// A context given to a park_* must be in no slot (one a take_* handed out, or a new one).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <mutex>

namespace mvs {

// read on every call: a process may switch the stash on and off between two calls
inline bool stash_enabled() { const char* e = getenv("MVS_KEEP_TABLE"); return !(e && e[0] == '0'); }

struct TableShape {
    uint32_t n_faces, n_views; uint64_t nnz;
    bool operator==(const TableShape& o) const { return n_faces == o.n_faces && n_views == o.n_views && nnz == o.nnz; }
};

struct StashTestAccess;
template <class Ctx, class Mutex = std::mutex>   // (the test's mutex knows its owner)
class Stash {
public:
    explicit Stash(void (*destroy)(Ctx*)) : destroy_(destroy) {}
    Stash(const Stash&) = delete;
    Stash& operator=(const Stash&) = delete;

    Ctx* take_spare() { std::lock_guard<Mutex> lock(m_); return take_spare_slot(); }
    // the context a data-cost call works on: the spare, else the one still parked with an OLD table (never two scenes resident at once), else null
    Ctx* take_working() { std::lock_guard<Mutex> lock(m_); return spare_ ? take_spare_slot() : take_table_slot(); }
    // cheap pre-check: may the parked table be the caller's?  (spares a fingerprint pass over a table that cannot match)
    bool shape_matches(const TableShape& shape) { std::lock_guard<Mutex> lock(m_); return table_ && shape_ == shape; }
    // the context parked with exactly this table, or null
    Ctx* take_table(uint64_t fp, const TableShape& shape) { std::lock_guard<Mutex> lock(m_); return table_ && fp_ == fp && shape_ == shape ? take_table_slot() : nullptr; }
    // parks `c`, table resident, for the view selection that follows
    void park_table(Ctx* c, uint64_t fp, const TableShape& shape) {
        Ctx* old;
        { std::lock_guard<Mutex> lock(m_); old = table_; table_ = c; fp_ = fp; shape_ = shape; }
        if (old) destroy_(old);
    }
    void park_spare(Ctx* c) {
        if (!c) return;
        Ctx* old;
        { std::lock_guard<Mutex> lock(m_); old = spare_; spare_ = c; }
        if (old) destroy_(old);
    }
    void release_all() {
        Ctx* a; Ctx* b;
        { std::lock_guard<Mutex> lock(m_); a = take_table_slot(); b = take_spare_slot(); }
        if (a) destroy_(a);
        if (b) destroy_(b);
    }

private:
    friend struct StashTestAccess;   // tests/cpp/test_stash.cpp: its destroy function checks that the mutex is not held
    // (mutex held) what the slot holds, which is then empty; a table slot without a context has no fingerprint
    Ctx* take_table_slot() { Ctx* c = table_; table_ = nullptr; fp_ = 0; return c; }
    Ctx* take_spare_slot() { Ctx* c = spare_; spare_ = nullptr; return c; }
    Mutex m_;
    void (*destroy_)(Ctx*);
    Ctx* table_ = nullptr; uint64_t fp_ = 0; TableShape shape_{0, 0, 0};   // a context whose device table has this fingerprint and shape
    Ctx* spare_ = nullptr;
};

}  // namespace mvs
