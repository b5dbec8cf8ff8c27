// comm.h -- the communicator as the sharded driver sees it (shard.hip and its shard_*.hip; the two implementations and the mvs_comm_*
// entry points are comm.hip): the mvs_comm interface, and what the ranks of a communicator whose devices address each other's memory
// publish for their peers (PeerSlot / PeerHub: the peer-push transport of shard_transport.hip).  Internal.
#pragma once
#include "ctx.h"

#include <atomic>
#include <memory>

// ---- peer-push transport (ranks that can address each other's device memory) ----
// What a rank publishes for its peers at the start of a solve: where ITS halo lives.  A sender gathers the boundary runs / labels of a
// colour phase out of its own arrays and stores them straight at their final places in the receiver's arrays (one kernel per phase,
// no staging buffers, no unpack launch); ordering is by stream events: a rank records one event per colour phase behind its push and
// waits -- on its stream, never on the host -- for the previous phase's events of the ranks it shares a cut with; the per-sweep
// energy pair is published the same way and summed by every rank on the device.  The host side of a wait only makes sure the
// event it is about to wait for has been RECORDED (enqueued) by its owner: a counter per rank, no device round trip.
struct PeerSlot {
    uint8_t* msg = nullptr; uint32_t* lab = nullptr; uint32_t stride = 0;             // message codes, decode buffers (2 x stride words)
    const uint32_t* msg_recv_idx = nullptr; const uint32_t* node_recv_idx = nullptr;   // device: where element k of a (phase, peer) chunk goes
    const uint64_t* msg_recv_off = nullptr; const uint64_t* node_recv_off = nullptr;   // host: [phase * P + peer] element offsets of the lists
    const uint64_t* msg_send_off = nullptr;                                            // host: the owner's SEND offsets (who shares a cut with whom)
    unsigned long long* energy = nullptr;                                              // device: [parity][2] the rank's share of a sweep's energy pair
    uint32_t* gain = nullptr; uint32_t* blab = nullptr; uint32_t* moved = nullptr;     // ICM: gains (as words), labels of the best labeling, [parity] nodes moved
    const uint32_t* all_recv_idx = nullptr; const uint64_t* all_recv_off = nullptr;    // every halo node, peer-major: device list, host offsets [peer]
    uint32_t phases = 0;
    std::vector<hipEvent_t> ev;                                                        // ring of phase events
};
struct PeerHub {
    int world;
    std::vector<PeerSlot> slot;
    std::unique_ptr<std::atomic<uint64_t>[]> recorded;     // events recorded by a rank in the current solve
    explicit PeerHub(int w) : world(w), slot(w), recorded(new std::atomic<uint64_t>[w]) { for (int r = 0; r < w; ++r) recorded[r].store(0); }
    ~PeerHub() { for (PeerSlot& p : slot) for (hipEvent_t e : p.ev) (void)hipEventDestroy(e); }
};

struct mvs_comm {
    int rank = 0, world = 1;
    virtual ~mvs_comm() {}
    // Failure of one rank must not leave the others waiting for it.  Every sharded entry point is a CALL that all ranks make in the
    // same order: begin_call() numbers it (the same number on every rank), fail() marks the current call as failed for everybody,
    // and a host-side wait inside the call (barrier, peer_wait) ends with an error once aborted() says so.  The mark names the call,
    // so the next call starts clean on every rank without anybody resetting anything.  Implemented by the in-process communicator; the
    // RCCL one keeps the no-ops below (a process that dies takes its group down through the launcher: see mvs_comm_abort in the header).
    uint64_t call_no = 0;
    virtual void begin_call() { ++call_no; }
    virtual void fail() {}
    virtual bool aborted() const { return false; }
    virtual void abort_all() {}          // the caller gives this communicator up (mvs_comm_abort): every rank's waits end with an error, for good
    virtual int device() const { return -1; }   // the device this rank's context has to live on (-1: any -- the communicator does not care)
    // non-null: the ranks can store into each other's device memory (PeerHub; the in-process communicator); barrier() = host rendezvous
    virtual PeerHub* peers() { return nullptr; }
    virtual void barrier() {}
    enum Type { U32, U64, F32 };
    enum Op { SUM, MAX };
    virtual void allreduce(void* buf, size_t n, Type t, Op op, hipStream_t s) = 0;          // in place, device buffer
    virtual void allgather(const void* send, void* recv, size_t bytes, hipStream_t s) = 0;  // recv = world x bytes
    // true: exchange is a world-wide rendezvous -- EVERY rank has to call it, also with nothing to send or receive (the in-process
    // communicator counts barriers over all ranks); false: point-to-point, a rank without traffic may skip the call
    virtual bool exchange_is_collective() const { return false; }
    // neighbour exchange of byte ranges: send + soff[q] .. soff[q + 1] goes to rank q, recv + roff[q] .. comes from rank q
    virtual void exchange(const uint8_t* send, const uint64_t* soff, uint8_t* recv, const uint64_t* roff, hipStream_t s) = 0;
    // two ranges per peer in ONE group (message bytes + label words of a colour phase: the sweep loop's Exchange, RCCL ranks only)
    virtual void exchange2(const uint8_t* sa, const uint64_t* soa, uint8_t* ra, const uint64_t* roa,
                           const uint8_t* sb, const uint64_t* sob, uint8_t* rb, const uint64_t* rob, hipStream_t s) {
        exchange(sa, soa, ra, roa, s); exchange(sb, sob, rb, rob, s);
    }
};
