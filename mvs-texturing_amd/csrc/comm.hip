// comm.hip -- the two communicators behind the mvs_comm interface (comm.h) and the mvs_comm_* entry points: RCCL (resolved with dlopen
// at run time, so the library carries no link-time dependency and shares whatever RCCL the process already loaded, e.g. PyTorch's) and
// an in-process one for `world` host threads whose devices address each other's memory.  The sharded driver (shard.hip) sees the
// interface only; which one it got decides the sweep loop's halo transport: in-process ranks push, RCCL ranks exchange.
#include "comm.h"
#include "call_barrier.h"
#include "shard_lists.h"

#include <rccl/rccl.h>
#include <dlfcn.h>

#include <mutex>

using namespace mvs;

namespace {

// ---- RCCL, resolved at run time ----
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl& rccl() {
    static Rccl R;
    static std::once_flag once;
    std::call_once(once, [] {
        // MVS_RCCL_LIB names the library to bind instead (tests: tests/tools/librccl_fake.so runs the ranks of this communicator as threads
        // sharing one device, so that the send / receive path below executes with real peers on a 1-GPU box); RTLD_LOCAL: its nccl* symbols
        // must not shadow those of an RCCL the process loaded already.  Otherwise the soname first: a process that already loaded an RCCL
        // (PyTorch ships its own next to its HIP runtime) gets that one.
        if (const char* over = getenv("MVS_RCCL_LIB")) { if (over[0]) { R.h = dlopen(over, RTLD_NOW | RTLD_LOCAL); if (!R.h) return; } }
        if (!R.h) for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { R.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (R.h) break; }
        if (!R.h) return;
#define MVS_SYM(f) R.f = reinterpret_cast<decltype(R.f)>(dlsym(R.h, "nccl" #f))
        MVS_SYM(GetUniqueId); MVS_SYM(CommInitRank); MVS_SYM(CommDestroy); MVS_SYM(AllReduce); MVS_SYM(AllGather); MVS_SYM(Send); MVS_SYM(Recv);
        MVS_SYM(GroupStart); MVS_SYM(GroupEnd); MVS_SYM(GetErrorString);
#undef MVS_SYM
    });
    if (!R.h || !R.GetUniqueId || !R.CommInitRank || !R.AllReduce || !R.AllGather || !R.Send || !R.Recv || !R.GroupStart || !R.GroupEnd)
        throw StatusError(MVS_ERR_UNSUPPORTED, "RCCL (librccl.so) is not available in this process");
    return R;
}
#define MVS_NCCL(expr)                                                                                               \
    do {                                                                                                             \
        ncclResult_t _r = (expr);                                                                                    \
        if (_r != ncclSuccess) throw HipError(std::string(#expr) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(_r) : "RCCL error")); \
    } while (0)

struct RcclComm : mvs_comm {
    ncclComm_t comm = nullptr;
    ~RcclComm() override { if (comm && rccl().CommDestroy) (void)rccl().CommDestroy(comm); }
    static ncclDataType_t dt(Type t) { return t == U32 ? ncclUint32 : t == U64 ? ncclUint64 : ncclFloat32; }
    void allreduce(void* buf, size_t n, Type t, Op op, hipStream_t s) override {
        MVS_NCCL(rccl().AllReduce(buf, buf, n, dt(t), op == SUM ? ncclSum : ncclMax, comm, s));
    }
    void allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        MVS_NCCL(rccl().AllGather(send, recv, bytes, ncclUint8, comm, s));
    }
    void post(const uint8_t* send, const uint64_t* soff, uint8_t* recv, const uint64_t* roff, hipStream_t s) {
        for (int q = 0; q < world; ++q) {   // actual neighbours only: empty ranges cost nothing
            if (q == rank) continue;
            if (soff[q + 1] > soff[q]) MVS_NCCL(rccl().Send(send + soff[q], soff[q + 1] - soff[q], ncclUint8, q, comm, s));
            if (roff[q + 1] > roff[q]) MVS_NCCL(rccl().Recv(recv + roff[q], roff[q + 1] - roff[q], ncclUint8, q, comm, s));
        }
    }
    void exchange(const uint8_t* send, const uint64_t* soff, uint8_t* recv, const uint64_t* roff, hipStream_t s) override {
        MVS_NCCL(rccl().GroupStart()); post(send, soff, recv, roff, s); MVS_NCCL(rccl().GroupEnd());
    }
    void exchange2(const uint8_t* sa, const uint64_t* soa, uint8_t* ra, const uint64_t* roa,
                   const uint8_t* sb, const uint64_t* sob, uint8_t* rb, const uint64_t* rob, hipStream_t s) override {
        MVS_NCCL(rccl().GroupStart()); post(sa, soa, ra, roa, s); post(sb, sob, rb, rob, s); MVS_NCCL(rccl().GroupEnd());
    }
};

// ---- in-process communicator: `world` host threads of ONE process, one per rank ----
// The ranks' contexts live on the devices named at creation: distinct GPUs of one node (the product's single-node route: peer access
// is switched on between all of them -- required --, halo data is STORED into the neighbours' arrays -- PeerHub -- and the collectives
// below are peer copies over xGMI) or one shared device (tests on a 1-GPU box: the same code, the ranks time-slice the device).
// Every collective is a rendezvous: post the pointers, barrier, copy (device to device, on the own stream, after the owner's "data
// ready" event), barrier, wait for the readers of the own send buffer.
__global__ void reduce_gathered_kernel(const uint8_t* __restrict__ gathered, size_t n, int world, int type /* 0 u32, 1 u64, 2 f32 */, int op /* 0 sum, 1 max */, void* __restrict__ out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (type == 0) { const uint32_t* g = (const uint32_t*)gathered; uint32_t a = 0; for (int q = 0; q < world; ++q) { const uint32_t v = g[(size_t)q * n + k]; a = op == 0 ? a + v : (v > a ? v : a); } ((uint32_t*)out)[k] = a; }
    else if (type == 1) { const unsigned long long* g = (const unsigned long long*)gathered; unsigned long long a = 0; for (int q = 0; q < world; ++q) { const unsigned long long v = g[(size_t)q * n + k]; a = op == 0 ? a + v : (v > a ? v : a); } ((unsigned long long*)out)[k] = a; }
    else { const float* g = (const float*)gathered; float a = g[k]; for (int q = 1; q < world; ++q) { const float v = g[(size_t)q * n + k]; a = op == 0 ? a + v : fmaxf(a, v); } ((float*)out)[k] = a; }   // rank order on every rank: identical sums
}
struct LocalHub {
    int world;
    std::vector<int> device;                 // device of rank r
    CallBarrier calls;                       // the ranks' rendezvous and its failure semantics (call_barrier.h: unit-tested on the CPU)
    std::vector<const uint8_t*> send; std::vector<const uint64_t*> soff;
    std::vector<hipEvent_t> ready, done;
    PeerHub peer;
    explicit LocalHub(int w) : world(w), device(w, 0), calls(w), send(w), soff(w), ready(w, nullptr), done(w, nullptr), peer(w) {}
    ~LocalHub() { for (hipEvent_t e : ready) if (e) (void)hipEventDestroy(e); for (hipEvent_t e : done) if (e) (void)hipEventDestroy(e); }
};
struct LocalComm : mvs_comm {
    std::shared_ptr<LocalHub> hub;
    DBuf<uint8_t> gathered;                  // all-reduce scratch (world x the operand) on this rank's device
    bool exchange_is_collective() const override { return true; }
    PeerHub* peers() override { return &hub->peer; }
    void barrier() override { hub->calls.arrive(call_no); }
    void begin_call() override { hub->calls.begin(++call_no); }
    void fail() override { hub->calls.fail(call_no); }
    bool aborted() const override { return hub->calls.abandoned(call_no); }
    void abort_all() override { hub->calls.abort_all(); }
    int device() const override { return hub->device[rank]; }
    void exchange(const uint8_t* send, const uint64_t* soff, uint8_t* recv, const uint64_t* roff, hipStream_t s) override {
        LocalHub& H = *hub;
        H.send[rank] = send; H.soff[rank] = soff;
        MVS_HIP(hipEventRecord(H.ready[rank], s));
        barrier();
        for (int q = 0; q < world; ++q) {
            if (q == rank) continue;
            MVS_HIP(hipStreamWaitEvent(s, H.ready[q], 0));
            const uint64_t n = roff[q + 1] - roff[q];
            if (n) {
                if (H.soff[q][rank + 1] - H.soff[q][rank] != n) throw HipError("local exchange: send / receive sizes disagree");
                MVS_HIP(hipMemcpyAsync(recv + roff[q], H.send[q] + H.soff[q][rank], n, hipMemcpyDefault, s));
            }
        }
        MVS_HIP(hipEventRecord(H.done[rank], s));
        barrier();
        for (int q = 0; q < world; ++q) if (q != rank) MVS_HIP(hipStreamWaitEvent(s, H.done[q], 0));   // my send buffers are free again
        barrier();   // nobody re-posts before everybody has queued its waits on this round's events
    }
    // every rank's `bytes` into every rank's recv (rank-major): peer copies, nothing through the host
    void allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        LocalHub& H = *hub;
        H.send[rank] = (const uint8_t*)send;
        MVS_HIP(hipEventRecord(H.ready[rank], s));
        barrier();
        for (int q = 0; q < world; ++q) {
            if (q != rank) MVS_HIP(hipStreamWaitEvent(s, H.ready[q], 0));
            if (bytes) MVS_HIP(hipMemcpyAsync((uint8_t*)recv + (size_t)q * bytes, H.send[q], bytes, hipMemcpyDefault, s));
        }
        MVS_HIP(hipEventRecord(H.done[rank], s));
        barrier();
        for (int q = 0; q < world; ++q) if (q != rank) MVS_HIP(hipStreamWaitEvent(s, H.done[q], 0));   // the peers have read `send`: it may change again
        barrier();
    }
    void allreduce(void* buf, size_t n, Type t, Op op, hipStream_t s) override {
        const size_t es = t == U64 ? 8 : 4, bytes = n * es;
        gathered.ensure((size_t)world * bytes + 16);
        allgather(buf, gathered.p, bytes, s);       // (returns with the waits for the peers' reads of `buf` queued: the kernel below may overwrite it)
        if (n) {
            hipLaunchKernelGGL(reduce_gathered_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint8_t*)gathered.p, n, world,
                               t == U32 ? 0 : t == U64 ? 1 : 2, op == SUM ? 0 : 1, buf);
            MVS_LAUNCH_CHECK();
        }
    }
};

}  // namespace

extern "C" {

mvs_status mvs_comm_unique_id(uint8_t id_out[MVS_COMM_ID_BYTES]) {
    if (!id_out) return api_fail(MVS_ERR_INVALID, "null argument");
    MVS_API_BEGIN
    static_assert(MVS_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    ncclUniqueId id;
    MVS_NCCL(rccl().GetUniqueId(&id));
    memcpy(id_out, id.internal, NCCL_UNIQUE_ID_BYTES);
    MVS_API_END
}

mvs_status mvs_comm_create_rccl(int device, int rank, int world, const uint8_t id[MVS_COMM_ID_BYTES], mvs_comm** out) {
    if (!id || !out || rank < 0 || rank >= world || world > MAX_PARTS) return api_fail(MVS_ERR_INVALID, "bad argument");
    *out = nullptr;
    MVS_API_BEGIN
    MVS_HIP(hipSetDevice(device));
    auto* c = new RcclComm; c->rank = rank; c->world = world;
    ncclUniqueId uid; memcpy(uid.internal, id, NCCL_UNIQUE_ID_BYTES);
    try { MVS_NCCL(rccl().CommInitRank(&c->comm, world, uid, rank)); } catch (...) { c->comm = nullptr; delete c; throw; }
    *out = c;
    MVS_API_END
}

/* `world` communicators for as many host threads of this process; rank r drives a context on devices[r] (NULL: all on the current
 * device).  Distinct devices get peer access switched on in both directions between every pair; a pair that cannot address each
 * other is MVS_ERR_UNSUPPORTED (one process per GPU over RCCL serves such a node). */
mvs_status mvs_comm_create_local_devices(int world, const int* devices, mvs_comm** out) {
    if (!out || world < 1 || world > MAX_PARTS) return api_fail(MVS_ERR_INVALID, "bad argument");
    MVS_API_BEGIN
    int cur = 0, ndev = 0;
    MVS_HIP(hipGetDevice(&cur));
    MVS_HIP(hipGetDeviceCount(&ndev));
    auto hub = std::make_shared<LocalHub>(world);
    for (int r = 0; r < world; ++r) {
        hub->device[r] = devices ? devices[r] : cur;
        if (hub->device[r] < 0 || hub->device[r] >= ndev) throw StatusError(MVS_ERR_INVALID, "bad device index");
    }
    struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{cur};
    for (int r = 0; r < world; ++r) {
        const int a = hub->device[r];
        MVS_HIP(hipSetDevice(a));
        MVS_HIP(hipEventCreateWithFlags(&hub->ready[r], hipEventDisableTiming));   // an event belongs to the device that is current when it is made
        MVS_HIP(hipEventCreateWithFlags(&hub->done[r], hipEventDisableTiming));
        for (int q = 0; q < world; ++q) {
            const int b = hub->device[q];
            if (b == a) continue;
            int can = 0;
            hipError_t e = hipDeviceCanAccessPeer(&can, a, b);
            if (e == hipSuccess) e = can ? hipDeviceEnablePeerAccess(b, 0) : hipErrorPeerAccessUnsupported;
            (void)hipGetLastError();
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                throw StatusError(MVS_ERR_UNSUPPORTED, "devices " + std::to_string(a) + " and " + std::to_string(b) + " cannot address each other's memory: "
                                  "run one process per GPU over RCCL (mvs_comm_create_rccl; bench.py --launch torchrun)");
        }
    }
    for (int r = 0; r < world; ++r) { auto* c = new LocalComm; c->rank = r; c->world = world; c->hub = hub; out[r] = c; }
    MVS_API_END
}
mvs_status mvs_comm_create_local(int world, mvs_comm** out) { return mvs_comm_create_local_devices(world, nullptr, out); }

/* gives the communicator up: every host-side wait of every rank inside a sharded call -- now or later -- ends with an error instead of
 * blocking (a rank's driver that dies OUTSIDE the library calls this so that its peers are released).  In-process communicators only. */
void mvs_comm_abort(mvs_comm* comm) { if (comm) comm->abort_all(); }

/* *peer_push = 1: the ranks of this communicator can store into each other's device memory (the in-process one): a solve of more than
 * one rank takes the peer-push transport */
mvs_status mvs_comm_info(mvs_comm* comm, int* rank, int* world, int* peer_push) {
    if (!comm) return api_fail(MVS_ERR_INVALID, "null argument");
    if (rank) *rank = comm->rank;
    if (world) *world = comm->world;
    if (peer_push) *peer_push = comm->peers() ? 1 : 0;
    return MVS_OK;
}

void mvs_comm_destroy(mvs_comm* comm) { delete comm; }

}  // extern "C"
