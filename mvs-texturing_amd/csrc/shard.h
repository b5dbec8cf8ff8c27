// shard.h -- what more than one source of the sharded driver needs (shard.hip: the entry points, shard_plan.hip: the halo plan,
// shard_table.hip: the sharded cost table, shard_transport.hip: the sweep loop's two halo transports): the partition, the shard object,
// the Transport interface and the prototypes these files call across.  Internal, host-and-device.  Something a single file uses stays
// in that file; the scheme as a whole is explained at the head of shard.hip.
#pragma once
#include "comm.h"
#include "shard_lists.h"

struct mvs_shard;

namespace mvs {

struct Parts { uint32_t b[MAX_PARTS + 1]; int n; };
__device__ __forceinline__ int part_of(const Parts& p, uint32_t i) { int q = 0; while (q + 1 < p.n && i >= p.b[q + 1]) ++q; return q; }

inline unsigned grid_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096)); }

// The steps of a solve (mvs_shard_view_selection) at which the two transports differ.  The communicator decides which one runs.
struct Transport {
    virtual ~Transport() {}
    virtual void start(mvs_shard*) {}                           // start of a solve: set-up and halo plan are in place
    virtual void before_phase(mvs_shard* S, uint32_t ph) = 0;   // the halo that colour phase `ph` reads has arrived
    virtual void after_boundary(mvs_shard* S, uint32_t ph) = 0; // the phase's boundary nodes are swept: their runs and labels leave
    virtual void sweep_energy(mvs_shard* S, int sweep) = 0;     // the sweep's energy pair over all ranks into the stop rule (mrf_step)
    virtual void icm_round(mvs_shard* S, int k) = 0;            // ICM round k: gains, moves, halo labels; all ranks' "moved" count into d_moved
    virtual void finish(mvs_shard*, int /*sweeps*/) {}          // the sweeps are queued
};

}  // namespace mvs

// ---------------------------------------------------------------------------------------------------------------
// the shard object
// ---------------------------------------------------------------------------------------------------------------
struct mvs_shard {
    mvs_ctx* ctx = nullptr; mvs_comm* comm = nullptr;
    mvs::Parts parts{}; int me = 0, P = 1; uint32_t F = 0, nb = 0, ne = 0;
    const uint32_t* d_adj_ptr = nullptr; const uint32_t* d_adj = nullptr; uint32_t E = 0;   // the adjacency lists in the LIBRARY's face order (see mvs_shard_create)
    mvs::DBuf<uint32_t> own_adj_ptr, own_adj;
    // Boundary-first colour phases: bnd marks the own nodes with a cut edge (from adjacency + partition alone: made once, at creation).  The
    // solver's schedule puts them in front of their colour class (mrf.h "zones"), a phase sweeps them first, hands their runs and
    // labels to the neighbours and sweeps the interior -- which reads nothing a peer writes -- while they travel.
    mvs::DBuf<uint8_t> bnd;
    mvs::DBuf<uint32_t> colours; bool colours_valid = false;   // the greedy colouring (a function of the pinned adjacency and the caller's ids): made by the first solve, kept
    // sharded table (global shape)
    mvs::DBuf<uint32_t> t_ptr; mvs::DBuf<uint16_t> t_view; mvs::DBuf<float> t_cost; mvs::DBuf<uint32_t> counts_g, keep, tmp_a, tmp_b, tmp_c;
    uint64_t nnz_global = 0;
    // plan scratch + lists
    mvs::DBuf<unsigned long long> k0, k1, k2, k3, v0, v1, ks, vs; mvs::DBuf<uint32_t> counters; mvs::DBuf<char> sort_tmp;
    struct Lists {
        mvs::DBuf<uint32_t> idx;            // message element indices (bytes) / node ids (words)
        std::vector<uint64_t> off;          // [phase][peer] -> element offset (size phases * P + 1)
        std::vector<uint64_t> bytes;        // [phase][peer] -> byte offset inside the phase's chunk (size phases * (P + 1)): Exchange's ranges
        uint64_t total = 0;
    } msg_send, msg_recv, node_send, node_recv, all_send, all_recv;   // all_*: every boundary / halo node, by (peer, id): ICM exchanges
    uint32_t phases = 0;
    mvs::DBuf<uint2> sbuf_col, rbuf_col;
    mvs::DBuf<unsigned long long> d_energy; mvs::DBuf<uint32_t> d_moved;
    double plan_ms = 0.0;
    // Everything that follows from (adjacency, partition, column LENGTHS of all faces) alone -- the shape of the sharded table, the
    // lists of boundary / halo columns, the halo plan of the solver -- is kept from one step to the next and reused while the
    // all-gathered column lengths stay what they were (compared on the device, one word read back): a scene that is solved again
    // (other images, other settings that keep the pattern, the steps of a benchmark) pays the planning once.
    mvs::DBuf<uint32_t> counts_prev; bool have_prev = false;
    Lists fs, fr; mvs::DBuf<uint32_t> pos_s, pos_r; std::vector<uint64_t> col_so, col_ro; uint64_t rec_s = 0, rec_r = 0;
    uint32_t nnz_l = 0, own_start = 0; bool tables_valid = false;
    bool plan_valid = false; uint32_t plan_colours = 0; uint64_t plan_total = 0; uint32_t plans_built = 0, plans_reused = 0;
    std::unique_ptr<mvs::Transport> xch, push; mvs::Transport* route = nullptr;   // the transports (Exchange, PeerPush), the one the last solve took
};

namespace mvs {

// ---- shard_plan.hip: sorted key lists on the device, and the solver's halo plan made of them ----
uint32_t own_directed_edges(mvs_shard* S);   // directed edges of the own faces (one read-back): the bound of every key list
void sort_pairs(mvs_shard* S, DBuf<unsigned long long>& k, DBuf<unsigned long long>* v, uint32_t n, hipStream_t s);
uint32_t unique_keys(mvs_shard* S, DBuf<unsigned long long>& k, uint32_t n, hipStream_t s);
void finish_node_list(mvs_shard* S, mvs_shard::Lists& L, DBuf<unsigned long long>& k, uint32_t n, uint32_t phases, hipStream_t s);
void build_plan(mvs_shard* S);               // S->phases and the six lists msg_* / node_* / all_* for the tables of the last mrf_setup

// ---- shard_table.hip: the steps of mvs_shard_data_costs, in the order every rank takes them ----
uint64_t shard_costs_over_ranks(mvs_shard* S, const mvs_settings* settings, mvs_dc_stats* stats);   // returns the own columns' entry count
void shard_gather_lengths(mvs_shard* S);                          // column lengths of all faces -> S->counts_g
bool shard_lengths_unchanged(mvs_shard* S, uint64_t* nnz_global); // ... are those of the previous step (and S->nnz_global; drains the stream)
void shard_rebuild_tables(mvs_shard* S);                          // face lists, local table's shape, record positions
void shard_fill_table(mvs_shard* S, uint64_t nnz_own);            // own block, halo columns through the communicator
void shard_activate_table(mvs_shard* S);                          // the context's active table := the sharded one

// ---- shard_transport.hip ----
std::unique_ptr<Transport> make_exchange();    // pack, grouped send / recv through the communicator, unpack
std::unique_ptr<Transport> make_peer_push();   // stores straight into the neighbours' arrays
void exchange_reserve(mvs_shard* S);                  // S->xch's staging buffers at the size of the plan just built
void exchange_nodes(mvs_shard* S, uint32_t* arr);     // a word per boundary node of `arr` to the neighbours' halo, through S->xch
void peer_push_info(const mvs_shard* S, uint64_t* phases_pushed, int* neighbours);   // S->push's counters (mvs_shard_transport_info)

}  // namespace mvs
