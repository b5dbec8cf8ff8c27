// k_mrf_setup.hip -- tex::view_selection on the GPU (libs/tex/view_selection.cpp:18-133), part 1 of 3: the solver's tables.
// k_mrf_sweep.hip has the sweeps, k_mrf_polish.hip whatever works on a labeling afterwards, mrf.h what they share.
//
// Model (restated from :27-82): node i = face, label set = {view_id + 1 : view_id
// in column i} with unaries = column costs, or the single label 0 when the column
// is empty; Potts edges of weight 1 between adjacent faces whose columns are both
// non-empty.  mapMAP (:93-118) is replaced by a GPU-resident tree-reweighted
// max-product solver -- colour-phased Gauss-Seidel sweeps (the adjacency graph is
// coloured, each colour class updates its messages in place in turn) + monotone
// ICM polish; the algorithm is specified to the float operation in DESIGN.md
// "MRF solver" and restated for the CPU in oracle/oracle.cpp -- labels are
// bit-identical by construction: a colour class is an independent set, min /
// argmin reductions are exact in any order, sums follow adjacency order,
// energies are 32.32 fixed-point integers.
#include "mrf.h"
#include "sort_scan.h"

namespace mvs {

namespace {

constexpr uint32_t MSG_BASE = MVS_MRF_MSG_BASE;   // first real message / map element (mvs_viewsel.h)

// ---- setup ----
// Node classes: the sweep is routed PER NODE, not per solve.  A node of degree <= 3 whose own column and whose in-model
// neighbours' columns hold at most 255 labels is a FAST node, swept with the lane-group width of its neighbourhood: G = 8 / 8 / 32 / 64
// lanes for kmx = max(K_i, K_j) <= 32 / 64 / 128 / 255 (classes 0 .. 3: mrf_sweep4_kernel<G>, class 1 mrf_sweep8_kernel with 8 labels
// per lane; the node's three outgoing runs are as long as the NEIGHBOURS' label lists, so they count).  Everything else -- a non-manifold
// edge (degree > 3), a column of more than 255 labels at the node or next to it -- is a GENERIC node (class 4): one wave per node, any
// degree, any K.  One non-manifold edge or one long column therefore costs a handful of generic nodes, not the whole solve, and the
// lane-group width follows the local column sizes instead of the largest column of the mesh.  A colour class is an independent set, so
// the order in which its nodes are swept -- hence the split into launches -- cannot change the result.
constexpr uint32_t CLS_GENERIC = 4;
__device__ __forceinline__ uint32_t mrf_node_class(uint32_t kmx, uint32_t deg, uint32_t force_generic) {
    if (force_generic || deg > 3u || kmx > 255u) return CLS_GENERIC;
    return kmx <= 32u ? 0u : kmx <= 64u ? 1u : kmx <= 128u ? 2u : 3u;
}
// (also rev[e] = position of the reverse directed edge (j -> i as an in-edge of j) of the in-edge e = (i <- j), 0xFFFFFFFF when the input is
//  asymmetric: found once here, read by the layout kernels below instead of being searched for again by each of them)
__global__ void mrf_size_kernel(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj,
                                uint32_t F, uint32_t pad_mask, uint32_t force_generic, uint32_t* __restrict__ size, uint8_t* __restrict__ cls,
                                uint32_t* __restrict__ maxes /* [0]=kmax [1]=degmax */, uint32_t* __restrict__ rev) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t k = 0, deg = 0;
    if (i < F) {
        k = col_ptr[i + 1] - col_ptr[i];
        const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
        deg = e1 - e0;
        uint32_t kmx = k;
        // four edges at a time, level by level (neighbour -> its column / its list bounds -> the head of its list): a thread's loads of one
        // level are independent of each other -- edge after edge this was a chain of 3 x 4 dependent round trips per node (0.11 ms at C3)
        for (uint32_t eb = e0; eb < e1; eb += 4) {
            uint32_t j[4], kj[4], r0[4], r1[4], head[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) j[q] = (eb + q < e1) ? adj[eb + q] : i;
#pragma unroll
            for (int q = 0; q < 4; ++q) { kj[q] = col_ptr[j[q] + 1] - col_ptr[j[q]]; r0[q] = adj_ptr[j[q]]; r1[q] = adj_ptr[j[q] + 1]; }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) head[q][t] = (r0[q] + t < r1[q]) ? adj[r0[q] + t] : 0xFFFFFFFFu;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (eb + q >= e1) continue;
                const uint32_t e = eb + q;
                size[e] = (k > 0 && kj[q] > 0) ? ((k + pad_mask) & ~pad_mask) : 0u;   // runs padded to a multiple of pad_mask + 1 elements
                if (k > 0) kmx = max(kmx, kj[q]);
                uint32_t r = 0xFFFFFFFFu;                         // the FIRST position of i in j's list
#pragma unroll
                for (int t = 3; t >= 0; --t) r = (head[q][t] == i) ? r0[q] + t : r;
                if (r == 0xFFFFFFFFu) { uint32_t rr = r0[q] + 4u; while (rr < r1[q] && adj[rr] != i) ++rr; if (rr < r1[q]) r = rr; }   // (degree > 4)
                rev[e] = r;
            }
        }
        cls[i] = (uint8_t)mrf_node_class(kmx, deg, force_generic);
    }
    for (int o = 32; o > 0; o >>= 1) { k = max(k, (uint32_t)__shfl_xor(k, o, 64)); deg = max(deg, (uint32_t)__shfl_xor(deg, o, 64)); }
    // same-address atomics serialise (~12 ns each): only waves that can still raise a maximum issue one
    if ((threadIdx.x & 63) == 0) {
        if (k > __hip_atomic_load(&maxes[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&maxes[0], k);
        if (deg > __hip_atomic_load(&maxes[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&maxes[1], deg);
    }
}

// ---- colour-phased schedule ----
// Greedy colouring of the adjacency graph in the order of the keys (hash32(i), i) -- the oracle's mrf_colour -- by
// Jones-Plassmann rounds: a node colours itself (smallest colour no smaller-key neighbour holds) as soon as all its
// smaller-key neighbours are coloured.  Larger-key neighbours are necessarily still uncoloured at that moment, so the
// result equals the sequential greedy colouring whatever the interleaving; only the number of rounds varies.
__device__ __forceinline__ uint32_t mrf_hash32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }
__device__ __forceinline__ bool mrf_key_less(uint32_t a, uint32_t b) { const uint32_t ha = mrf_hash32(a), hb = mrf_hash32(b); return ha != hb ? ha < hb : a < b; }
constexpr uint32_t NO_COLOUR = 0xFFFFFFFFu;
__global__ void mrf_colour_init_kernel(uint32_t* __restrict__ colour, uint32_t* __restrict__ iota, uint32_t F) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < F) { colour[i] = NO_COLOUR; iota[i] = i; }
}
// `orig` (null: identity) = the caller's id of every node: the keys are those of the CALLER's numbering, so the colouring -- hence the
// labeling -- does not depend on the order the library keeps the nodes in (ctx.h "the library's own mesh layout").
__global__ void mrf_colour_round_kernel(const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj, const uint32_t* __restrict__ orig, uint32_t F,
                                        uint32_t* colour, uint32_t* __restrict__ pending) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F) return;
    if (__hip_atomic_load(colour + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != NO_COLOUR) return;
    unsigned long long used = 0ull;
    bool ready = true;
    const uint32_t oi = orig ? orig[i] : i;
    const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
    for (uint32_t eb = e0; eb < e1 && ready; eb += 4) {      // four neighbours at a time: their ids, keys and colours are independent loads
        uint32_t j[4], oj[4], cj[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) j[t] = (eb + t < e1) ? adj[eb + t] : i;
#pragma unroll
        for (int t = 0; t < 4; ++t) { oj[t] = orig ? orig[j[t]] : j[t]; cj[t] = __hip_atomic_load(colour + j[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (j[t] == i || !mrf_key_less(oj[t], oi)) continue;   // (a padded slot is the node itself)
            if (cj[t] == NO_COLOUR) ready = false; else used |= 1ull << cj[t];
        }
    }
    if (ready) {
        // 64 colours in use around one node: the mask (and the 6-bit class sort) cannot hold a 65th -- reported, not wrapped
        if (used == ~0ull) { pending[1] = 1u; used = 0ull; }
        __hip_atomic_store(colour + i, (uint32_t)__builtin_ctzll(~used), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else *pending = 1u;                                       // racing stores of the same value
}
// the sort key of the schedule order: 2 * sub-class + zone (mrf.h)
__global__ void mrf_sortkey_kernel(const uint32_t* __restrict__ colour, const uint8_t* __restrict__ cls, const uint8_t* __restrict__ bnd, uint32_t F, uint32_t* __restrict__ key) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < F) { const uint32_t c = colour[i], k = cls[i]; key[i] = 2u * ((k == CLS_GENERIC) ? SUB_GENERIC + c : 4u * c + k) + ((bnd && bnd[i]) ? 0u : 1u); }
}
// sub_begin[k] = first position of a key >= k in the sorted key array, k = 0 .. N_KEY
__global__ void mrf_sub_begin_kernel(const uint32_t* __restrict__ sorted, uint32_t F, uint32_t* __restrict__ sub_begin) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > N_KEY) return;
    uint32_t lo = 0, hi = F;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sorted[mid] < c) lo = mid + 1; else hi = mid; }
    sub_begin[c] = lo;
}
// Message layout, SENDER-major: the runs a node WRITES (one per out-edge, in its list order, each as long as the
// receiver's padded label count) are contiguous, and nodes follow each other in (colour, id) order.  A colour phase
// therefore streams its previous-outgoing reads and its stores through one contiguous region (2 of the 3 message
// accesses per label); only the incoming reads gather 1 run out of each neighbour's block.
// size[e] belongs to the in-edge e = (i <- j) of its receiver i; the out-edge r = (j -> i) of j owns the same run.
// nsz[b * (F + 1) + q] = message elements node perm[q] sends to receivers of colour b (b < n_col; with n_col == 1 all
// receivers count as colour 0 = plain sender-major).  One exclusive scan over the n_col * (F + 1) entries then yields the
// layout  [receiver colour][sender in (colour, id) order][out-edge in list order]:
//   * what a phase WRITES (and re-reads for damping) is one contiguous stream per receiver colour;
//   * what a phase READS as incoming messages is the whole super-region of its own colour -- every byte of it is consumed
//     in that phase, by receivers that follow each other roughly in memory order, so no fetched line is wasted (a plain
//     sender-major layout gathers one 90-byte run out of each neighbour's 270-byte block: 2x the bytes at C3).
constexpr int MAX_LAYOUT_COLOURS = 8;
__global__ void mrf_nodesize_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ colour, const uint32_t* __restrict__ adj_ptr,
                                    const uint32_t* __restrict__ adj, const uint32_t* __restrict__ size, const uint32_t* __restrict__ rev, uint32_t F, uint32_t n_col,
                                    uint32_t* __restrict__ nsz) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > F) return;
    uint32_t acc[MAX_LAYOUT_COLOURS];
#pragma unroll
    for (int b = 0; b < MAX_LAYOUT_COLOURS; ++b) acc[b] = 0;
    if (q < F) {
        const uint32_t j = perm[q];
        const uint32_t ra = adj_ptr[j], rz = adj_ptr[j + 1];
        for (uint32_t rb = ra; rb < rz; rb += 4) {           // four out-edges at a time: the loads of a level are independent
            uint32_t i[4], e[4], b[4], sz[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { const bool on = rb + t < rz; i[t] = on ? adj[rb + t] : j; e[t] = on ? rev[rb + t] : 0xFFFFFFFFu; }   // e = (i <- j): the in-edge of the receiver that owns this run
#pragma unroll
            for (int t = 0; t < 4; ++t) { b[t] = (n_col > 1) ? colour[i[t]] : 0u; sz[t] = (e[t] != 0xFFFFFFFFu) ? size[e[t]] : 0u; }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int c = 0; c < MAX_LAYOUT_COLOURS; ++c) acc[c] += ((uint32_t)c == b[t]) ? sz[t] : 0u;
        }
    }
#pragma unroll
    for (int b = 0; b < MAX_LAYOUT_COLOURS; ++b) if ((uint32_t)b < n_col) nsz[(size_t)b * (F + 1) + q] = acc[b];
}
__global__ void mrf_inoff_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ colour, const uint32_t* __restrict__ adj_ptr,
                                 const uint32_t* __restrict__ adj, const uint32_t* __restrict__ size, const uint32_t* __restrict__ rev, const uint32_t* __restrict__ noff,
                                 uint32_t F, uint32_t n_col, uint32_t* __restrict__ in_off) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= F) return;
    const uint32_t j = perm[q];
    uint32_t off[MAX_LAYOUT_COLOURS];
#pragma unroll
    for (int b = 0; b < MAX_LAYOUT_COLOURS; ++b) off[b] = ((uint32_t)b < n_col) ? noff[(size_t)b * (F + 1) + q] : 0u;
    const uint32_t ra = adj_ptr[j], rz = adj_ptr[j + 1];
    for (uint32_t rb = ra; rb < rz; rb += 4) {               // four out-edges at a time (see mrf_nodesize_kernel); offsets are handed out in list order
        uint32_t i[4], e[4], b[4], sz[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { const bool on = rb + t < rz; i[t] = on ? adj[rb + t] : j; e[t] = on ? rev[rb + t] : 0xFFFFFFFFu; }
#pragma unroll
        for (int t = 0; t < 4; ++t) { b[t] = (n_col > 1) ? colour[i[t]] : 0u; sz[t] = (e[t] != 0xFFFFFFFFu) ? size[e[t]] : 0u; }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (e[t] == 0xFFFFFFFFu) continue;
            uint32_t o = 0;
#pragma unroll
            for (int c = 0; c < MAX_LAYOUT_COLOURS; ++c) { if ((uint32_t)c == b[t]) { o = off[c]; off[c] += sz[t]; } }
            in_off[e[t]] = o;
        }
    }
}

// ---- view-set bitmaps: a column as W = ceil(V / 64) words (dmath.h "view-set bitmaps") ----
// bits[i * W + w] = word w of column i's bitmap, built from the table mrf_setup is handed, every call: one streaming pass over the view
// ids, 16 lanes per node, the words collected in the group's LDS tile (a group never spans waves and LDS operations of a wave execute
// in order: no barrier).  The set-up's questions about a NEIGHBOUR's list -- is it the same list, where does view v sit in it -- are
// then answered from W words instead of from the list (mrf_edge_kernel, mrf_record_bits_kernel, mrf_map_bits_kernel).
// That rests on strictly ascending ids below V.  The library's own tables have them; a caller's table (mvs_ctx_costs_upload) is taken as
// it is, so every id is bound-checked before its bit is set and every adjacent pair is compared: *flag is raised for a table that breaks
// the rule, and mrf_setup then keeps to the list kernels, whose behaviour on such input is what it always was.
constexpr uint32_t BITMAP_MAX_WORDS = 16;   // V <= 1024: one word per lane of a node's group (64 MB at 2 M faces x 200 views; beyond: the list kernels)
// A lane takes FOUR consecutive entries per pass (one 8-byte load of view ids at 2-byte alignment, one 16-byte load of costs at 4-byte
// alignment -- global loads need no natural alignment on gfx950), so a column of up to 64 entries is one pass of its group and all its
// loads are in flight at once; one entry per lane made these kernels wait for three dependent rounds of 32-byte requests per column.
// The last three entries of the table are read one by one: a wide load there would pass the end of the array.
template <class T> __device__ __forceinline__ T ld_unaligned(const void* p) { T v; __builtin_memcpy(&v, p, sizeof(T)); return v; }
__device__ __forceinline__ void ld_views4(const uint16_t* __restrict__ view_id, uint64_t at, uint32_t n, uint64_t nnz, uint32_t (&v)[4]) {
    if (at + 4u <= nnz) { const uint2 w = ld_unaligned<uint2>(view_id + at); v[0] = w.x & 0xFFFFu; v[1] = w.x >> 16; v[2] = w.y & 0xFFFFu; v[3] = w.y >> 16; }
    else {
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) v[r] = (r < n) ? (uint32_t)view_id[at + r] : 0u;
    }
}
__global__ void __launch_bounds__(256) mrf_bitmap_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, uint64_t nnz, uint32_t F, uint32_t V, uint32_t W,
                                                         unsigned long long* __restrict__ bits, uint32_t* __restrict__ flag) {
    __shared__ uint32_t s_b[16][2 * BITMAP_MAX_WORDS];
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t gl = threadIdx.x & 15;
    if (i >= F) return;
    uint32_t* tile = s_b[threadIdx.x >> 4];
    tile[2 * gl] = 0u; tile[2 * gl + 1] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
    bool bad = false;
    uint32_t carry = 0u;                                        // the last id of the previous pass
    for (uint32_t t0 = 0; t0 < K; t0 += 64) {
        const uint32_t t = t0 + 4u * gl, n = t < K ? min(K - t, 4u) : 0u;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (n) ld_views4(view_id, (uint64_t)p0 + t, n, nnz, v);
        uint32_t before = (uint32_t)__shfl_up((int)v[3], 1, 16);   // (a lane with entries has a left neighbour with four)
        if (gl == 0u) before = carry;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            if (r < n) {
                bad = bad || v[r] >= V || ((t + r) != 0u && before >= v[r]);
                if (v[r] < V) atomicOr(&tile[v[r] >> 5], 1u << (v[r] & 31u));
            }
            before = v[r];
        }
        carry = (uint32_t)__shfl((int)v[3], 15, 16);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (gl < W) bits[(size_t)i * W + gl] = (unsigned long long)tile[2 * gl] | ((unsigned long long)tile[2 * gl + 1] << 32);
    if (bad) *flag = 1u;                                        // racing stores of the same value
}

// (bits != null -- the bitmap route: ident[e] = 1 iff the two label lists of the valid edge e of a FAST node are identical, i.e. the two
//  bitmaps are equal; what mrf_ident_kernel finds by comparing the lists)
__global__ void mrf_edge_kernel(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj,
                                uint32_t F, const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ size, const uint32_t* __restrict__ rev, MrfEdge* __restrict__ edge,
                                const uint8_t* __restrict__ cls, const unsigned long long* __restrict__ bits, uint32_t W, uint8_t* __restrict__ ident) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F) return;
    const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
    const bool fast = bits && cls[i] != CLS_GENERIC;           // only fast nodes have records
    for (uint32_t eb = e0; eb < e1; eb += 4) {               // four edges at a time: the loads of a level are independent
        uint32_t j[4], r[4], io[4], sz[4], oo[4], kj[4];
        unsigned long long diff[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int t = 0; t < 4; ++t) { const bool on = eb + t < e1; j[t] = on ? adj[eb + t] : i; r[t] = on ? rev[eb + t] : 0xFFFFFFFFu; io[t] = on ? in_off[eb + t] : 0u; sz[t] = on ? size[eb + t] : 0u; }
#pragma unroll
        for (int t = 0; t < 4; ++t) { oo[t] = (r[t] != 0xFFFFFFFFu) ? in_off[r[t]] : 0u; kj[t] = col_ptr[j[t] + 1] - col_ptr[j[t]]; }
        if (fast)
            for (uint32_t w = 0; w < W; ++w) {
                const unsigned long long own = bits[(size_t)i * W + w];
#pragma unroll
                for (int t = 0; t < 4; ++t) diff[t] |= own ^ bits[(size_t)j[t] * W + w];
            }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (eb + t >= e1) continue;
            const bool has = r[t] != 0xFFFFFFFFu;
            MrfEdge m;
            m.in_off = MSG_BASE + io[t];                       // [0, MSG_BASE) is the reserved zero / identity run
            m.out_off = has ? MSG_BASE + oo[t] : 0u;
            m.kj = (sz[t] > 0 && has) ? kj[t] : 0u;
            edge[eb + t] = m;
            if (bits) ident[eb + t] = (uint8_t)((fast && m.kj != 0u && diff[t] == 0ull) ? 1u : 0u);
        }
    }
}

// map[in_off(e) + t] = position of L_i[t] in L_j (binary search; lists ascending, calculate_data_costs.cpp:272), for the in-edges
// e = (i <- j) whose SENDER j is a generic node: the generic sweep kernel re-aligns its outgoing runs through these 16-bit maps
// (fast senders carry byte maps in their records).
constexpr uint32_t MAP_TILE = 256;   // neighbour lists up to this length are searched in LDS
__global__ void __launch_bounds__(256) mrf_map_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const uint32_t* __restrict__ adj_ptr,
                               const uint32_t* __restrict__ adj, uint32_t F, const MrfEdge* __restrict__ edge, const uint8_t* __restrict__ cls, uint16_t* __restrict__ map) {
    // 16 lanes per node.  The binary search is a chain of dependent loads: through global memory it is latency bound,
    // so the neighbour's list is first copied (coalesced) into the group's LDS tile.  A group never spans
    // waves and LDS operations of a wave execute in order, so the tile needs no barrier.
    __shared__ uint16_t s_l[16][MAP_TILE];
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t gl = threadIdx.x & 15;
    if (i >= F) return;
    uint16_t* tile = s_l[threadIdx.x >> 4];
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
    for (uint32_t e = adj_ptr[i]; e < adj_ptr[i + 1]; ++e) {
        const MrfEdge m = edge[e];
        if (m.kj == 0 || cls[adj[e]] != CLS_GENERIC) continue;  // group-uniform
        const uint32_t q0 = col_ptr[adj[e]];
        const bool in_lds = m.kj <= MAP_TILE;                  // group-uniform
        if (in_lds) for (uint32_t t = gl; t < m.kj; t += 16) tile[t] = view_id[q0 + t];
        for (uint32_t t = gl; t < K; t += 16) {
            const uint16_t key = view_id[p0 + t];
            uint32_t lo = 0, hi = m.kj;
            if (in_lds) { while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (tile[mid] < key) lo = mid + 1; else hi = mid; } }
            else { while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (view_id[q0 + mid] < key) lo = mid + 1; else hi = mid; } }
            const uint16_t found = (lo < m.kj) ? (in_lds ? tile[lo] : view_id[q0 + lo]) : (uint16_t)0;
            map[m.in_off + t] = (lo < m.kj && found == key) ? (uint16_t)lo : MAP_NONE;
        }
    }
}

// ---- fast nodes (degree <= 3, columns of the neighbourhood <= 255 labels): per-node RECORDS + 48-byte descriptors ----
// The sweep streams, per node and in (colour, id) order, ONE read-only record instead of gathering from the CSR:
//   [ceil4(K) label words: cost code << 16 | view id]  [for every out-edge whose two label lists differ: ceil4(K_j) map bytes]
// padded to a multiple of four words.  A phase reads a contiguous run of records: no partially used lines (a phase used to
// read every third column of the CSR), the view id of the decoded label is already in a register (no gather), the unaries
// are 16-bit fixed point (2 instead of 4 bytes; part of the solver's definition, restated in oracle/oracle.cpp), the
// re-alignment maps are bytes (K <= 255; 0xFF = label absent at the sender) and exist only where the lists differ.
constexpr uint32_t REC_BASE = MRF_REC_BASE;   // words [0, REC_BASE) of the record array are zero: where masked lanes load
// ident[e] = 1 iff the two label lists of the (valid) directed edge e are identical; 16 lanes per node.  The kernel is a chain
// of dependent gathers (edge -> neighbour -> its column -> its view ids), so three edges are in flight at a time.
// (Round 5 tried the symmetry -- of a pair only the node with the smaller id compares the lists and writes both flags: half the list
// gathers, but three more dependent look-ups per edge in front of them: 0.375 -> 0.52 ms.  Reverted.)
__global__ void __launch_bounds__(256) mrf_ident_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const uint32_t* __restrict__ adj_ptr,
                                                        const uint32_t* __restrict__ adj, uint32_t F, const MrfEdge* __restrict__ edge, const uint8_t* __restrict__ cls,
                                                        uint8_t* __restrict__ ident) {
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t gl = threadIdx.x & 15;
    if (i >= F || cls[i] == CLS_GENERIC) return;               // only fast nodes have records
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
    const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
    for (uint32_t e = e0; e < e1; e += 3) {
        uint32_t kj[3], q0[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool on = e + k < e1;
            kj[k] = on ? edge[e + k].kj : 0u;
            q0[k] = col_ptr[on ? adj[e + k] : i];
        }
        uint32_t same = 0;   // bit k: edge e + k still looks identical
#pragma unroll
        for (int k = 0; k < 3; ++k) same |= (kj[k] != 0u && kj[k] == K) ? (1u << k) : 0u;
        if (same) {          // group-uniform
            for (uint32_t t = gl; t < K; t += 16) {
                const uint32_t v = view_id[p0 + t];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if ((same >> k) & 1u) { if (view_id[q0[k] + t] != v) same &= ~(1u << k); }
            }
            for (int o = 8; o > 0; o >>= 1) same &= __shfl_xor(same, o, 16);
        }
        if (gl < 3 && e + gl < e1 && kj[gl] != 0u) ident[e + gl] = (uint8_t)((same >> gl) & 1u);
    }
}

// ---- the record and descriptor format of the fast nodes: written down here, used by the four set-up kernels below (mrf_recsize_kernel,
// mrf_record_kernel, mrf_desc_kernel, mrf_record_bits_kernel) and by nothing else -- the sweep kernels decode with arithmetic of their own ----
// A map byte is the SLOT of the sweep kernel's LDS tile that holds the sender's label: the tile is row-major over r = label mod 4
// (slot = (at & 3) * G + (at >> 2) for position `at` in the sender's list, G = 8 << class lanes per node), so that the lanes of a
// group read consecutive banks.  "Label absent at the sender" is the +inf slot 4 * G; for G = 64 the slots fill the byte range
// 0 .. 254 and 0xFF marks absence (the kernel steers it to slot 256).
// (a class-1 node -- mrf_sweep8_kernel: 8 lanes x 8 labels -- has the tile row-major over label mod 8: slot = (at & 7) * 8 + (at >> 3),
//  "absent" = slot 64, and its map sections padded to 8 bytes: its lanes read 8 map bytes at once)
struct RecLayout {
    bool w8; uint32_t rs /* row stride of the tile */, none_byte /* "absent" */, lmask, lshift;
    __device__ __forceinline__ explicit RecLayout(uint32_t cls)
        : w8(cls == 1u), rs(w8 ? 8u : 8u << cls), none_byte(w8 ? 64u : (cls < 3u ? 4u * rs : 0xFFu)), lmask(w8 ? 7u : 3u), lshift(w8 ? 3u : 2u) {}
    __device__ __forceinline__ uint32_t slot(uint32_t at) const { return (at & lmask) * rs + (at >> lshift); }                // map byte of position `at`
    __device__ __forceinline__ uint32_t map_words(uint32_t kj) const { return w8 ? 2u * ((kj + 7u) >> 3) : (kj + 3u) >> 2; }  // words of a map of kj bytes
};
__device__ __forceinline__ uint32_t label_word(float c, uint32_t view) { return (cost_code(c) << 16) | view; }
// The descriptor of fast node i: K labels, record at word rec_off behind REC_BASE (none for an empty column), and per slot d < 3 the edge
// words m[d], "identical label lists" ident[d], the neighbour nb[d] (the node itself where there is none: a valid index, masked by kj = 0
// wherever it is used) and "that neighbour has a lower colour" low[d].  An edge that is not in the model (beyond the degree, an empty
// column at either end) gets kj = 0 and the offsets of the reserved zero run.
__device__ __forceinline__ NodeDesc make_desc(uint32_t i, uint32_t K, uint32_t rec_off, uint32_t deg, const MrfEdge (&m)[3], const uint32_t (&ident)[3],
                                              const uint32_t (&nb)[3], const uint32_t (&low)[3]) {
    NodeDesc nd;
    nd.rec = K ? REC_BASE + rec_off : 0u; nd.id = i; nd.kk = K;
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d) {
        const bool on = d < deg && K != 0u && m[d].kj != 0u;
        const uint32_t flag_low = (d < deg && low[d]) ? 1u : 0u, flag_ident = (on && ident[d]) ? 1u : 0u;
        nd.in_off[d] = (on ? m[d].in_off : 0u) | flag_low; nd.out_off[d] = (on ? m[d].out_off : 0u) | flag_ident;
        nd.kk |= (on ? m[d].kj : 0u) << (8 + 8 * d); nd.nbr[d] = nb[d];
    }
    return nd;
}

// rsz[q] = words of the record of node perm[q] (rsz[F] = 0)
// qpos[i] = position of node i in the (colour, id) order (the inverse of perm)
__global__ void mrf_recsize_kernel(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ adj_ptr, const MrfEdge* __restrict__ edge,
                                   const uint8_t* __restrict__ ident, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ perm, uint32_t F,
                                   uint32_t* __restrict__ rsz, uint32_t* __restrict__ qpos) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > F) return;
    uint32_t w = 0;
    if (q < F) {
        const uint32_t i = perm[q], K = col_ptr[i + 1] - col_ptr[i];
        qpos[i] = q;
        if (K && cls[i] != CLS_GENERIC) {
            w = (K + 3u) & ~3u;
            const RecLayout L(cls[i]);
            const uint32_t e0 = adj_ptr[i], e1 = adj_ptr[i + 1];
            for (uint32_t eb = e0; eb < e1; eb += 4) {       // four edges at a time: independent loads
                uint32_t kj[4], id[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) { const bool on = eb + t < e1; kj[t] = on ? edge[eb + t].kj : 0u; id[t] = on ? ident[eb + t] : 1u; }
#pragma unroll
                for (int t = 0; t < 4; ++t) if (kj[t] && !id[t]) w += L.map_words(kj[t]);
            }
            w = (w + 3u) & ~3u;
        }
    }
    rsz[q] = w;
}
// fills the record of node i: 16 lanes per node, nodes in FACE order -- the columns are read as one sequential stream (in the
// (colour, id) order of the records a pass would touch every fourth column), the records are written where they belong;
// the node's own list sits in an LDS tile for the searches (a group never spans waves and LDS operations of a wave
// execute in order: no barrier)
__global__ void __launch_bounds__(256) mrf_record_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                         const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj, const MrfEdge* __restrict__ edge,
                                                         const uint8_t* __restrict__ ident, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ qpos, const uint32_t* __restrict__ roff,
                                                         uint32_t F, uint32_t* __restrict__ rec) {
    __shared__ uint16_t s_l[16][256];
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t gl = threadIdx.x & 15;
    if (i >= F) return;
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
    const uint32_t ci = cls[i];
    if (K == 0 || ci == CLS_GENERIC) return;
    const RecLayout L(ci);
    const uint32_t q = qpos[i];
    uint16_t* tile = s_l[threadIdx.x >> 4];
    uint32_t* out = rec + REC_BASE + roff[q];
    const uint32_t K4 = (K + 3u) & ~3u;
    // the (at most three: a fast node) edges' sizes, flags and neighbour columns are requested before the column is read, not one edge
    // after the other behind it
    const uint32_t e0 = adj_ptr[i], deg = adj_ptr[i + 1] - e0;
    uint32_t kj3[3], q03[3];
    {
        uint32_t kj[3], idn[3], nb[3];
#pragma unroll
        for (uint32_t d = 0; d < 3; ++d) { const bool on = d < deg; kj[d] = on ? edge[e0 + d].kj : 0u; idn[d] = on ? (uint32_t)ident[e0 + d] : 1u; nb[d] = on ? adj[e0 + d] : i; }
#pragma unroll
        for (uint32_t d = 0; d < 3; ++d) { kj3[d] = (kj[d] != 0u && idn[d] == 0u) ? kj[d] : 0u; q03[d] = col_ptr[nb[d]]; }
    }
    for (uint32_t t = gl; t < K4; t += 16) {
        uint32_t w = 0u;
        if (t < K) { const uint32_t v = view_id[p0 + t]; tile[t] = (uint16_t)v; w = label_word(cost[p0 + t], v); }
        out[t] = w;
    }
    uint32_t pos = K4;
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d) {
        const uint32_t kj = kj3[d];
        if (kj == 0) continue;                                 // group-uniform: not in the model, or identical lists (no map)
        const uint32_t q0 = q03[d], nw = L.map_words(kj);
        for (uint32_t wI = gl; wI < nw; wI += 16) {
            // positions of the RECEIVER's labels 4 wI .. 4 wI + 3 in this (the sender's) list: four lower-bound searches in
            // lockstep (the step count depends on K only), so their LDS reads are independent
            uint32_t key[4], lo[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) { const uint32_t t2 = 4u * wI + r; key[r] = (t2 < kj) ? (uint32_t)view_id[q0 + t2] : 0xFFFFFFFFu; }
            for (uint32_t n = K; n > 1u;) {
                const uint32_t half = n >> 1;
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) lo[r] += ((uint32_t)tile[lo[r] + half - 1u] < key[r]) ? half : 0u;
                n -= half;
            }
            uint32_t word = 0u;
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) {
                // lo = the last candidate position: the key sits there, or one further (beyond the list), or nowhere
                uint32_t at = lo[r] + (((uint32_t)tile[lo[r]] < key[r]) ? 1u : 0u);
                const uint32_t byte = (at < K && (uint32_t)tile[at < K ? at : 0u] == key[r]) ? L.slot(at) : L.none_byte;
                word |= byte << (8 * r);
            }
            out[pos + wI] = word;
        }
        pos += nw;
    }
    for (uint32_t t = pos + gl; t < ((pos + 3u) & ~3u); t += 16) out[t] = 0u;
}
__global__ void mrf_desc_kernel(const uint32_t* __restrict__ col_ptr, const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj,
                                const MrfEdge* __restrict__ edge, const uint8_t* __restrict__ ident, const uint32_t* __restrict__ perm,
                                const uint32_t* __restrict__ colour, const uint32_t* __restrict__ roff, uint32_t n_fast, NodeDesc* __restrict__ desc) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;   // position in the schedule order; the fast nodes come first
    if (q >= n_fast) return;
    const uint32_t i = perm[q];
    const uint32_t k = col_ptr[i + 1] - col_ptr[i];
    const uint32_t e0 = adj_ptr[i], deg = adj_ptr[i + 1] - e0, ci = colour[i];
    MrfEdge m[3]; uint32_t idn[3], nb[3], low[3];
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d) {
        m[d].in_off = 0u; m[d].out_off = 0u; m[d].kj = 0u; idn[d] = 0u; low[d] = 0u; nb[d] = i;
        if (d < deg) { nb[d] = adj[e0 + d]; low[d] = (colour[nb[d]] < ci) ? 1u : 0u; }
        if (d < deg && k > 0) {
            m[d] = edge[e0 + d];
            // the message written over out-edge d is aligned with the neighbour's list: identity iff the lists are equal
            // (a symmetric property, so the in-edge's flag serves)
            idn[d] = (m[d].kj && ident[e0 + d]) ? 1u : 0u;
        }
    }
    desc[q] = make_desc(i, k, roff[q], deg, m, idn, nb, low);
}

// ---- the bitmap route of the two kernels above and of mrf_map_kernel: the same bytes, no neighbour list is read ----
// a bitmap word per lane -> the group's LDS tile: the words and, beside them, the number of views in the words below each (an exclusive
// scan over the group's 16 lanes), which is what a rank or a select needs besides the word itself
__device__ __forceinline__ void bitmap_to_tile(unsigned long long word, uint32_t gl, unsigned long long* __restrict__ t_bits, uint32_t* __restrict__ t_pre) {
    const uint32_t c = bitmap_popc(word);
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 16); incl += (gl >= (uint32_t)o) ? up : 0u; }
    t_bits[gl] = word; t_pre[gl] = incl - c;
}
// Record AND descriptor of node i, 16 lanes per node, nodes in face order (see mrf_record_kernel).  The map of out-edge d holds, for
// every label of the RECEIVER nb[d] in its list order, the slot of that label in THIS node's list.  The receiver's labels are the set
// bits of its bitmap in ascending order: lane gl finds the first of its group of four from the word counts (bitmap_select) and walks on
// from there; the position of view v in the own list is the number of own bits below v (bitmap_rank_word).  Slot formulas, the "absent"
// byte and the padding are RecLayout's, as in mrf_record_kernel -- the records are the same bytes.
// The group also has everything the node's descriptor is made of (edge words, identity flags, roff[q]) in registers: lane 0 writes it;
// the neighbours' colours are requested together with the edge words.  Nodes with an empty column have a descriptor and no record.
__global__ void __launch_bounds__(256) mrf_record_bits_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost,
                                                              const uint32_t* __restrict__ adj_ptr, const uint32_t* __restrict__ adj, const MrfEdge* __restrict__ edge,
                                                              const uint8_t* __restrict__ ident, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ qpos, const uint32_t* __restrict__ roff,
                                                              const uint32_t* __restrict__ colour, const unsigned long long* __restrict__ bits, uint32_t W, uint64_t nnz, uint32_t F, uint32_t n_fast,
                                                              uint32_t* __restrict__ rec, NodeDesc* __restrict__ desc) {
    __shared__ unsigned long long s_bits[16][4][BITMAP_MAX_WORDS];   // [group][own, receiver 0 .. 2][word]
    __shared__ uint32_t s_pre[16][4][BITMAP_MAX_WORDS];
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t gl = threadIdx.x & 15;
    if (i >= F) return;
    const uint32_t ci = cls[i];
    if (ci == CLS_GENERIC) return;                             // (a fast node: degree <= 3)
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
    const uint32_t q = qpos[i], ro = roff[q], col_i = colour[i];
    const uint32_t e0 = adj_ptr[i], deg = min(adj_ptr[i + 1] - e0, 3u);
    MrfEdge m[3]; uint32_t idn[3], nb[3], low[3], kj3[3];
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d) {
        const bool on = d < deg;
        m[d].in_off = on ? edge[e0 + d].in_off : 0u; m[d].out_off = on ? edge[e0 + d].out_off : 0u; m[d].kj = on ? edge[e0 + d].kj : 0u;
        idn[d] = on ? (uint32_t)ident[e0 + d] : 0u; nb[d] = on ? adj[e0 + d] : i;
    }
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d) {
        low[d] = (colour[nb[d]] < col_i) ? 1u : 0u;
        kj3[d] = (K == 0u || idn[d]) ? 0u : m[d].kj;            // a map only where the edge is in the model and the lists differ
    }
    const bool maps = (kj3[0] | kj3[1] | kj3[2]) != 0u;         // group-uniform
    unsigned long long bw[4] = {0ull, 0ull, 0ull, 0ull};
    if (maps && gl < W) {
        bw[0] = bits[(size_t)i * W + gl];
#pragma unroll
        for (uint32_t d = 0; d < 3; ++d) if (kj3[d]) bw[d + 1] = bits[(size_t)nb[d] * W + gl];
    }
    if (gl == 0u && q < n_fast) desc[q] = make_desc(i, K, ro, deg, m, idn, nb, low);
    if (K == 0u) return;
    const RecLayout L(ci);
    uint32_t* out = rec + REC_BASE + ro;
    const uint32_t K4 = (K + 3u) & ~3u;
    for (uint32_t t = 4u * gl; t < K4; t += 64) {             // (records start at multiples of four words: 16-byte stores)
        const uint32_t n = min(K - t, 4u);
        const uint64_t at = (uint64_t)p0 + t;
        uint32_t v[4]; float c[4];
        ld_views4(view_id, at, n, nnz, v);
        if (at + 4u <= nnz) { const float4 cc = ld_unaligned<float4>(cost + at); c[0] = cc.x; c[1] = cc.y; c[2] = cc.z; c[3] = cc.w; }
        else {
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) c[r] = (r < n) ? cost[at + r] : 0.0f;
        }
        uint4 w;
        w.x = label_word(c[0], v[0]);
        w.y = (n > 1u) ? label_word(c[1], v[1]) : 0u;
        w.z = (n > 2u) ? label_word(c[2], v[2]) : 0u;
        w.w = (n > 3u) ? label_word(c[3], v[3]) : 0u;
        *reinterpret_cast<uint4*>(out + t) = w;
    }
    uint32_t pos = K4;
    if (maps) {
        unsigned long long (*t_bits)[BITMAP_MAX_WORDS] = s_bits[threadIdx.x >> 4];
        uint32_t (*t_pre)[BITMAP_MAX_WORDS] = s_pre[threadIdx.x >> 4];
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) bitmap_to_tile(bw[b], gl, t_bits[b], t_pre[b]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
        for (uint32_t d = 0; d < 3; ++d) {
            const uint32_t kj = kj3[d];
            if (kj == 0u) continue;                            // group-uniform: not in the model, or identical lists (no map)
            const uint32_t nw = L.map_words(kj);
            for (uint32_t wI = gl; wI < nw; wI += 16) {
                const uint32_t n = 4u * wI;                    // the receiver's labels n .. n + 3
                uint32_t word = L.none_byte * 0x01010101u;
                if (n < kj) {
                    uint32_t w = 0u;                           // the last word with at most n views below it holds label n
                    for (uint32_t ww = 1u; ww < W; ++ww) w = (t_pre[d + 1][ww] <= n) ? ww : w;
                    unsigned long long x = t_bits[d + 1][w];
                    x &= ~bitmap_below(bitmap_select(x, n - t_pre[d + 1][w]));
                    word = 0u;
#pragma unroll
                    for (uint32_t r = 0; r < 4; ++r) {
                        uint32_t byte = L.none_byte;
                        if (n + r < kj) {
                            while (x == 0ull && w + 1u < W) { ++w; x = t_bits[d + 1][w]; }
                            if (x != 0ull) {
                                const uint32_t p = (uint32_t)__builtin_ctzll(x);
                                x &= x - 1ull;
                                const uint32_t at = bitmap_rank_word(t_bits[0][w], t_pre[0][w], p);   // position of that view in the own list
                                if (at != BITMAP_NONE) byte = L.slot(at);
                            }
                        }
                        word |= byte << (8 * r);
                    }
                }
                out[pos + wI] = word;
            }
            pos += nw;
        }
    }
    for (uint32_t t = pos + gl; t < ((pos + 3u) & ~3u); t += 16) out[t] = 0u;
}
// mrf_map_kernel on the bitmap route: the position of L_i[t] in the generic sender's list = its rank in the sender's bitmap
__global__ void __launch_bounds__(256) mrf_map_bits_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const uint32_t* __restrict__ adj_ptr,
                                                           const uint32_t* __restrict__ adj, uint32_t F, const MrfEdge* __restrict__ edge, const uint8_t* __restrict__ cls,
                                                           const unsigned long long* __restrict__ bits, uint32_t W, uint16_t* __restrict__ map) {
    __shared__ unsigned long long s_bits[16][BITMAP_MAX_WORDS];
    __shared__ uint32_t s_pre[16][BITMAP_MAX_WORDS];
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t gl = threadIdx.x & 15;
    if (i >= F) return;
    unsigned long long* t_bits = s_bits[threadIdx.x >> 4];
    uint32_t* t_pre = s_pre[threadIdx.x >> 4];
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
    for (uint32_t e = adj_ptr[i]; e < adj_ptr[i + 1]; ++e) {
        const MrfEdge m = edge[e];
        const uint32_t j = adj[e];
        if (m.kj == 0 || cls[j] != CLS_GENERIC) continue;      // group-uniform
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the previous edge's reads of the tile)
        bitmap_to_tile(gl < W ? bits[(size_t)j * W + gl] : 0ull, gl, t_bits, t_pre);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (uint32_t t = gl; t < K; t += 16) {
            const uint32_t v = view_id[p0 + t], w = v >> 6;
            const uint32_t at = (w < W) ? bitmap_rank_word(t_bits[w], t_pre[w], v) : BITMAP_NONE;
            map[m.in_off + t] = (at != BITMAP_NONE) ? (uint16_t)at : MAP_NONE;
        }
    }
}

// argmin-unary start (max_sweeps == 0): sel / lab / selcost of every node
__global__ void mrf_argmin_unary_kernel(const uint32_t* __restrict__ col_ptr, const uint16_t* __restrict__ view_id, const float* __restrict__ cost, uint32_t F,
                                        uint32_t* __restrict__ sel, uint32_t* __restrict__ lab, float* __restrict__ selcost) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= F) return;
    const uint32_t p0 = col_ptr[i], K = col_ptr[i + 1] - p0;
    uint32_t bt = 0;
    for (uint32_t t = 1; t < K; ++t) if (cost[p0 + t] < cost[p0 + bt]) bt = t;
    sel[i] = bt;
    lab[i] = K ? (uint32_t)view_id[p0 + bt] + 1u : 0u;
    selcost[i] = K ? cost[p0 + bt] : 1.0f;
}

}  // namespace

constexpr uint32_t RUN_PAD_MASK = 7;      // message runs padded to multiples of 8 elements: the 8-byte stores of mrf_sweep8_kernel (the 4-label kernels need 4)

// ---- mrf_setup, stage by stage ----
// what the stages of one set-up share (on the stack)
struct Setup {
    hipStream_t s; uint32_t F, E /* directed edges */, W /* bitmap words per face */; unsigned nb /* blocks of 256 nodes */;
    uint32_t force_generic;
    bool bitmaps;                     // the bitmap route; setup_read_sizes has the last word
    const unsigned long long* bits;   // ctx->m_bits.p once the route is settled and it is the bitmap route, else null
    uint32_t* pending;                // [0] a node is still waiting for a colour, [1] a node saw all 64 colours around it
    uint32_t* maxes;                  // [0] kmax, [1] degmax, [2] message total, [3] a column is not strictly ascending
};
static dim3 groups16(uint32_t F) { return dim3((unsigned)(((size_t)F * 16 + 255) / 256)); }   // 16 lanes per node, blocks of 256 threads

static void setup_check_params(const mvs_mrf_params* params) {
    if (!(params->rho > 0.0f && params->rho <= 1.0f) || !(params->damping >= 0.0f && params->damping < 1.0f))
        throw StatusError(MVS_ERR_INVALID, "mrf params: need 0 < rho <= 1, 0 <= damping < 1");
    // window < 1 would index the energy history out of bounds (hist[sweep - window]); the others are nonsensical when negative
    if (params->window < 1 || params->min_sweeps < 0 || !(params->min_improvement >= 0.0f) || params->icm_iters < 0)
        throw StatusError(MVS_ERR_INVALID, "mrf params: need window >= 1, min_sweeps >= 0, min_improvement >= 0, icm_iters >= 0");
}

// the number of directed edges, the per-edge arrays sized by it, and the set-up's device words cleared
static Setup setup_edge_count(mvs_ctx* ctx) {
    Setup S{};
    S.s = ctx->stream; S.F = ctx->csr_faces; S.E = ctx->r_adj_edges; S.nb = (S.F + 255) / 256;
    if (!ctx->r_adj_edges_known) {   // lists handed over on the device and used as they are: their length is only known there
        MVS_HIP(hipMemcpyAsync(&S.E, ctx->r_adj_ptr + S.F, sizeof(uint32_t), hipMemcpyDeviceToHost, S.s));
        MVS_HIP(hipStreamSynchronize(S.s));
    }
    ctx->m_size.ensure((size_t)S.E + 2); ctx->m_edge.ensure((size_t)S.E + 1);
    ctx->m_n_adj = S.E;
    S.pending = &ctx->words->colour_pending; S.maxes = &ctx->words->setup_kmax;
    MVS_HIP(hipMemsetAsync(S.pending, 0, 6 * sizeof(uint32_t), S.s));   // the colouring's two words and the four behind them
    MVS_HIP(hipMemsetAsync(ctx->m_size.p, 0, ((size_t)S.E + 2) * sizeof(uint32_t), S.s));
    // degenerate inputs (fewer than four table entries, no edge at all) take the generic kernel throughout; "mrf_force_generic" is a test hook
    S.force_generic = (ctx->csr_nnz < 4 || S.E == 0 || ctx->mrf_force_generic) ? 1u : 0u;
    return S;
}

// view-set bitmaps of the table as it is handed in (whatever made it: this context's data costs, an upload, pruning, a shard's face
// range), built anew every call; the word behind the two maxima says whether the table keeps the rule they rest on.  More than
// BITMAP_MAX_WORDS words per face, or "mrf_force_lists" (a test hook): the list kernels.
static void setup_bitmaps(mvs_ctx* ctx, Setup& S) {
    S.W = bitmap_words(ctx->csr_views);
    S.bitmaps = S.F && S.W >= 1 && S.W <= BITMAP_MAX_WORDS && !ctx->mrf_force_lists;
    if (!S.bitmaps) return;
    ctx->m_bits.ensure((size_t)S.F * S.W + 1);
    hipLaunchKernelGGL(mrf_bitmap_kernel, groups16(S.F), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_view, (uint64_t)ctx->csr_nnz, S.F, ctx->csr_views, S.W,
                       ctx->m_bits.p, S.maxes + 3);
    MVS_LAUNCH_CHECK();
}

// run sizes, reverse edges, node classes, the two maxima
static void setup_sizes_and_classes(mvs_ctx* ctx, const Setup& S) {
    ctx->m_cls.ensure((size_t)S.F + 4);
    ctx->m_rev.ensure((size_t)S.E + 2);
    if (!S.F) return;
    hipLaunchKernelGGL(mrf_size_kernel, dim3(S.nb), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_adj_ptr, ctx->r_adj, S.F, RUN_PAD_MASK, S.force_generic,
                       ctx->m_size.p, ctx->m_cls.p, S.maxes, ctx->m_rev.p);
    MVS_LAUNCH_CHECK();
}

// ---- colour-phased schedule: colouring (Jones-Plassmann rounds), nodes in (colour, id) order ----
static void setup_colouring(mvs_ctx* ctx, const Setup& S) {
    const size_t F = S.F;
    ctx->m_colour.ensure(F + 2); ctx->m_perm.ensure(F + 2);
    ctx->m_tmp_a.ensure((size_t)MAX_LAYOUT_COLOURS * (F + 1) + 72); ctx->m_tmp_b.ensure((size_t)MAX_LAYOUT_COLOURS * (F + 1) + 2);
    ctx->m_tmp_c.ensure(F + 2);
    ctx->m_colours = 0; ctx->m_sub_begin.assign(N_KEY + 1, 0); ctx->m_n_fast = 0; ctx->m_range_q.clear(); ctx->m_range_nb = ctx->m_range_ne = 0;
    ctx->m_sweep_no = 0; ctx->m_last_phase = 0xFFFFFFFFu;
    if (!S.F) return;
    hipLaunchKernelGGL(mrf_colour_init_kernel, dim3(S.nb), dim3(256), 0, S.s, ctx->m_colour.p, ctx->m_tmp_a.p /* iota */, S.F); MVS_LAUNCH_CHECK();
    // a sharded caller hands in the colouring it kept from its first solve (the colours follow from the adjacency alone, which a
    // shard pins at creation, like its layout): no rounds
    if (ctx->m_colour_in) MVS_HIP(hipMemcpyAsync(ctx->m_colour.p, ctx->m_colour_in, F * sizeof(uint32_t), hipMemcpyDeviceToDevice, S.s));
    for (int round = 0; !ctx->m_colour_in; ++round) {
        if (round >= 4096) throw StatusError(MVS_ERR_HIP, "graph colouring did not terminate");
        MVS_HIP(hipMemsetAsync(S.pending, 0, sizeof(uint32_t), S.s));
        // a batch of rounds per read-back: 16 first (meshes of 0.2 - 2 M faces need 12 - 16 rounds; a round past the eighth costs 4 - 10 us -- coloured
        // nodes leave at their first load -- a read-back 25 us of an idle device), then 4
        for (int k = 0; k < (round == 0 ? 16 : 4); ++k) {
            hipLaunchKernelGGL(mrf_colour_round_kernel, dim3(S.nb), dim3(256), 0, S.s, ctx->r_adj_ptr, ctx->r_adj, ctx->t_perm, S.F, ctx->m_colour.p, S.pending);
            MVS_LAUNCH_CHECK();
        }
        uint32_t hp[2] = {0, 0};   // set if any round of the batch left a node waiting
        read_words(ctx, S.pending, hp, 2);
        if (hp[1]) throw StatusError(MVS_ERR_UNSUPPORTED, "adjacency graph needs more than 64 colours (a node with >= 64 mutually constrained neighbours)");
        if (!hp[0]) break;
    }
}

// stable sort of the node ids by sub-class key: perm = the schedule order; every (colour, class) pair is a contiguous range
static void setup_schedule_order(mvs_ctx* ctx, const Setup& S) {
    if (!S.F) return;
    hipLaunchKernelGGL(mrf_sortkey_kernel, dim3(S.nb), dim3(256), 0, S.s, ctx->m_colour.p, ctx->m_cls.p, ctx->m_bnd, S.F, ctx->m_tmp_c.p); MVS_LAUNCH_CHECK();
    dev_sort_pairs(ctx->sort_tmp, S.s, ctx->m_tmp_c.p, ctx->m_tmp_b.p, ctx->m_tmp_a.p, ctx->m_perm.p, S.F, 0, 10);
    ctx->m_sub.ensure(3 * (size_t)N_KEY + 8);   // [0, N_KEY]: sub_begin; behind it the own-share ranges of sub_range()
    hipLaunchKernelGGL(mrf_sub_begin_kernel, dim3((N_KEY + 256) / 256), dim3(256), 0, S.s, ctx->m_tmp_b.p, S.F, ctx->m_sub.p); MVS_LAUNCH_CHECK();
    read_block(ctx, ctx->m_sub.p, ctx->m_sub_begin.data(), (N_KEY + 1) * sizeof(uint32_t));
    const std::vector<uint32_t>& sb = ctx->m_sub_begin;
    uint32_t C = 0;   // colours 0 .. C-1 are in use (greedy colours are dense)
    for (uint32_t c = 0; c < 64; ++c)
        if (sb[2 * (4 * c + 4)] > sb[2 * (4 * c)] || sb[2 * (SUB_GENERIC + c + 1)] > sb[2 * (SUB_GENERIC + c)]) C = c + 1;
    ctx->m_colours = C;
    ctx->m_n_fast = sb[2 * SUB_GENERIC];
}

// message layout (sender-major, (colour, id) node order): in_off[e] for every directed edge e (adjacency order), returned; the total
// lands behind the two maxima (one read-back).  Edges whose reverse is missing (asymmetric input) keep offset 0 and are disabled by
// mrf_edge_kernel.
// in_off lives in m_sel2 until setup_edge_table has read it: everything that reads it is queued on this stream ahead of the memsets of
// setup_solver_state (and a re-allocation frees through hipFree, which waits for the device), so no host synchronisation is needed
// before that stage takes the buffer back.
static const uint32_t* setup_message_layout(mvs_ctx* ctx, const Setup& S) {
    DBuf<uint32_t>& in_off = ctx->m_sel2;
    in_off.ensure(std::max<size_t>((size_t)S.E + 2, (size_t)S.F + 2));
    MVS_HIP(hipMemsetAsync(in_off.p, 0, ((size_t)S.E + 2) * sizeof(uint32_t), S.s));
    if (!S.F) { MVS_HIP(hipMemsetAsync(S.maxes + 2, 0, sizeof(uint32_t), S.s)); return in_off.p; }
    // the offsets are 32 bits wide: the total is bounded by 3 (degree) x (entries + 3 pad per column) on a manifold; beyond
    // 2^32 the scan below would wrap silently, so large inputs get an exact 64-bit total first
    if ((uint64_t)S.E * 4ull + 4ull * (uint64_t)ctx->csr_nnz >= 0xFFFFFFF0ull) {
        const uint64_t total = sum_u32(ctx, ctx->m_size.p, (size_t)S.E + 1);
        if ((uint64_t)MSG_BASE + total >= 0xFFFFFFF0ull)
            throw StatusError(MVS_ERR_UNSUPPORTED, "message array exceeds 2^32 elements (shard the graph: DESIGN.md multi-GPU)");
    }
    const uint32_t n_col = (ctx->m_colours >= 2 && ctx->m_colours <= (uint32_t)MAX_LAYOUT_COLOURS) ? ctx->m_colours : 1u;
    const size_t n_ent = (size_t)n_col * ((size_t)S.F + 1);
    ctx->m_tmp_a.ensure(n_ent + 72); ctx->m_tmp_b.ensure(n_ent + 2);
    hipLaunchKernelGGL(mrf_nodesize_kernel, dim3((S.F + 256) / 256), dim3(256), 0, S.s, ctx->m_perm.p, ctx->m_colour.p, ctx->r_adj_ptr, ctx->r_adj,
                       ctx->m_size.p, ctx->m_rev.p, S.F, n_col, ctx->m_tmp_a.p);
    MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, ctx->m_tmp_a.p, ctx->m_tmp_b.p, n_ent, nullptr);   // the last entry of every colour segment is 0, so scan[last] = total
    hipLaunchKernelGGL(mrf_inoff_kernel, dim3(S.nb), dim3(256), 0, S.s, ctx->m_perm.p, ctx->m_colour.p, ctx->r_adj_ptr, ctx->r_adj,
                       ctx->m_size.p, ctx->m_rev.p, ctx->m_tmp_b.p, S.F, n_col, in_off.p);
    MVS_LAUNCH_CHECK();
    MVS_HIP(hipMemcpyAsync(S.maxes + 2, ctx->m_tmp_b.p + (n_ent - 1), sizeof(uint32_t), hipMemcpyDeviceToDevice, S.s));
    return in_off.p;
}

// the one read-back of {kmax, degmax, total, unsorted}; it also settles the route
static void setup_read_sizes(mvs_ctx* ctx, Setup& S) {
    uint32_t hm[4];
    read_words(ctx, S.maxes, hm, 4);
    if (hm[3]) S.bitmaps = false;   // (a column that is not strictly ascending below csr_views)
    ctx->m_bitmaps = S.bitmaps;
    S.bits = S.bitmaps ? ctx->m_bits.p : nullptr;
    ctx->m_total = (uint64_t)MSG_BASE + hm[2]; ctx->m_kmax = hm[0]; ctx->m_degmax = hm[1];
    if (ctx->m_total >= 0xFFFFFFF0ull) throw StatusError(MVS_ERR_UNSUPPORTED, "message array exceeds 2^32 elements");
}

// the edge words, from in_off (setup_message_layout: still in m_sel2); on the bitmap route the "identical label lists" flags with them
static void setup_edge_table(mvs_ctx* ctx, const Setup& S, const uint32_t* in_off) {
    ctx->m_ident.ensure((size_t)S.E + 1);
    if (!S.bitmaps) MVS_HIP(hipMemsetAsync(ctx->m_ident.p, 0, (size_t)S.E + 1, S.s));   // (the bitmap route's edge kernel writes every flag)
    if (!S.F) return;
    hipLaunchKernelGGL(mrf_edge_kernel, dim3(S.nb), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_adj_ptr, ctx->r_adj, S.F, in_off, ctx->m_size.p, ctx->m_rev.p,
                       ctx->m_edge.p, ctx->m_cls.p, S.bits, S.W, ctx->m_ident.p);
    MVS_LAUNCH_CHECK();
}

// records + descriptors of the fast nodes
static void setup_fast_records(mvs_ctx* ctx, const Setup& S) {
    const uint32_t F = S.F, n_fast = ctx->m_n_fast;
    if (!n_fast) return;
    // upper bound of the record array (no read-back): labels nnz + 3 F, maps <= one byte per message element; incl. slack for reads past the last record
    const size_t rec_cap = (size_t)REC_BASE + ctx->csr_nnz + 8 * (size_t)F + ctx->m_total / 4 + (size_t)ctx->m_n_adj + 1024;
    ctx->m_rec.ensure(rec_cap);
    MVS_HIP(hipMemsetAsync(ctx->m_rec.p, 0, REC_BASE * sizeof(uint32_t), S.s));
    if (!S.bitmaps) {
        hipLaunchKernelGGL(mrf_ident_kernel, groups16(F), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_view, ctx->r_adj_ptr, ctx->r_adj, F,
                           ctx->m_edge.p, ctx->m_cls.p, ctx->m_ident.p);
        MVS_LAUNCH_CHECK();
    }
    uint32_t* rsz = ctx->m_tmp_a.p; uint32_t* roff = ctx->m_tmp_b.p; uint32_t* qpos = ctx->m_tmp_c.p;   // F + 1 entries each
    hipLaunchKernelGGL(mrf_recsize_kernel, dim3((F + 256) / 256), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_adj_ptr, ctx->m_edge.p, ctx->m_ident.p,
                       ctx->m_cls.p, ctx->m_perm.p, F, rsz, qpos);
    MVS_LAUNCH_CHECK();
    exclusive_scan_u32(ctx, rsz, roff, (size_t)F + 1, nullptr);
    ctx->m_desc.ensure((size_t)F + 1);
    if (S.bitmaps) {   // records and descriptors in one pass
        hipLaunchKernelGGL(mrf_record_bits_kernel, groups16(F), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->r_adj_ptr, ctx->r_adj,
                           ctx->m_edge.p, ctx->m_ident.p, ctx->m_cls.p, qpos, roff, ctx->m_colour.p, S.bits, S.W, (uint64_t)ctx->csr_nnz, F, n_fast,
                           ctx->m_rec.p, ctx->m_desc.p);
        MVS_LAUNCH_CHECK();
        return;
    }
    hipLaunchKernelGGL(mrf_record_kernel, groups16(F), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_view, ctx->r_cost, ctx->r_adj_ptr, ctx->r_adj,
                       ctx->m_edge.p, ctx->m_ident.p, ctx->m_cls.p, qpos, roff, F, ctx->m_rec.p);
    MVS_LAUNCH_CHECK();
    hipLaunchKernelGGL(mrf_desc_kernel, dim3((n_fast + 255) / 256), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_adj_ptr, ctx->r_adj, ctx->m_edge.p,
                       ctx->m_ident.p, ctx->m_perm.p, ctx->m_colour.p, roff, n_fast, ctx->m_desc.p);
    MVS_LAUNCH_CHECK();
}

// 16-bit re-alignment maps of the runs the generic nodes SEND (indexed like the messages); only those elements are ever read
static void setup_generic_maps(mvs_ctx* ctx, const Setup& S) {
    if (S.F == ctx->m_n_fast) return;
    ctx->m_map.ensure(ctx->m_total + 8);
    if (S.bitmaps)
        hipLaunchKernelGGL(mrf_map_bits_kernel, groups16(S.F), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_view, ctx->r_adj_ptr, ctx->r_adj, S.F,
                           ctx->m_edge.p, ctx->m_cls.p, S.bits, S.W, ctx->m_map.p);
    else
        hipLaunchKernelGGL(mrf_map_kernel, groups16(S.F), dim3(256), 0, S.s, ctx->r_ptr, ctx->r_view, ctx->r_adj_ptr, ctx->r_adj, S.F,
                           ctx->m_edge.p, ctx->m_cls.p, ctx->m_map.p);
    MVS_LAUNCH_CHECK();
    ctx->pq.ensure(ctx->csr_nnz + 1);   // scratch row per generic node (the data-cost work buffer is free by now)
}

// zeroed messages, the two decode buffers and the start labeling; returns the solver's progress record at sweep 0
static mvs_mrf_progress setup_decode_buffers(mvs_ctx* ctx, const Setup& S, const mvs_mrf_params* params) {
    hipStream_t s = S.s;
    ctx->m_msg_a.ensure(ctx->m_total + 1024);   // slack: lanes beyond a run read on (up to 4 * 64 elements)
    MVS_HIP(hipMemsetAsync(ctx->m_msg_a.p, 0, (ctx->m_total + 1024) * sizeof(msg_t), s));   // zero codes, incl. the reserved zero run
    // decode buffers: two of F + 1 entries each (see ctx.h)
    const size_t F1 = (size_t)S.F + 1;
    ctx->m_stride = (uint32_t)F1;
    ctx->m_sel.ensure(2 * F1); ctx->m_lab.ensure(2 * F1); ctx->m_cost.ensure(2 * F1);
    ctx->m_sel2.ensure(F1); ctx->m_cand.ensure(F1); ctx->m_gain.ensure(F1);
    MVS_HIP(hipMemsetAsync(ctx->m_sel.p, 0, 2 * F1 * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(ctx->m_lab.p, 0, 2 * F1 * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(ctx->m_cost.p, 0, 2 * F1 * sizeof(float), s));
    // start state = argmin-unary decode everywhere: only needed when no sweep runs (ICM-only); otherwise the first
    // sweep (and, when sharded, the halo exchange that follows it) defines every label that is ever read
    mvs_mrf_progress init; memset(&init, 0, sizeof(init)); init.best = ~0ull; init.energy = ~0ull; init.w = 0u; init.best_w = 1u;
    if (S.F && params->max_sweeps <= 0) {
        hipLaunchKernelGGL(mrf_argmin_unary_kernel, dim3(S.nb), dim3(256), 0, s, ctx->r_ptr, ctx->r_view, ctx->r_cost, S.F, ctx->m_sel.p, ctx->m_lab.p, ctx->m_cost.p);
        MVS_LAUNCH_CHECK();
        init.w = 1u; init.best_w = 0u;
    }
    ctx->b_sel = ctx->m_sel.p + init.best_w * F1; ctx->b_lab = ctx->m_lab.p + init.best_w * F1; ctx->b_cost = ctx->m_cost.p + init.best_w * F1;
    ctx->best_resolved = true;
    MVS_HIP(hipMemsetAsync(ctx->m_gain.p, 0, F1 * sizeof(float), s));
    return init;
}

// energy partials, and the device-side solver state: sweep 0, best = hist[0] = 2^64 - 1
static void setup_solver_state(mvs_ctx* ctx, const Setup& S, const mvs_mrf_params* params, const mvs_mrf_progress& init) {
    hipStream_t s = S.s;
    // energy partials: [0, 4) the reduced pair; then 2 x EPART_BLOCKS per colour phase (sweep kernels) / 2 x 2048 (energy kernel)
    const size_t epart = 4 + 2 * (size_t)EPART_BLOCKS * std::max<size_t>(ctx->m_colours, 1);
    ctx->m_energy.ensure(epart);
    MVS_HIP(hipMemsetAsync(ctx->m_energy.p, 0, epart * sizeof(unsigned long long), s));   // slots a phase never writes stay zero
    ctx->m_state.ensure(1); ctx->m_hist.ensure((size_t)std::max(params->max_sweeps, 0) + 2);
    ensure_report_ring(ctx);
    ctx->seq_base += ctx->steps_issued;   // sequence numbers of this solve: seq_base + step (never reused within the context)
    ctx->h_ring[mvs_ctx::RING] = init;   // staging slot for the upload
    MVS_HIP(hipMemcpyAsync(ctx->m_state.p, &ctx->h_ring[mvs_ctx::RING], sizeof(init), hipMemcpyHostToDevice, s));
    // the step kernel's own counter: steps of this solve so far, and the solve's sequence base (staged in the pinned words behind the slots' sequence numbers)
    ctx->m_ctl.ensure(4);
    uint32_t* stage = ctx->h_seq + (mvs_ctx::RING + mvs_ctx::ICM_RING);
    stage[0] = 0u; stage[1] = ctx->seq_base;
    MVS_HIP(hipMemcpyAsync(ctx->m_ctl.p, stage, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    MVS_HIP(hipMemsetAsync(ctx->m_hist.p, 0xFF, sizeof(unsigned long long), s));
    ctx->steps_issued = 0; ctx->icm_dirty_valid = false; ctx->exact_valid = false;
}

// Builds the solver's edge tables for the active CSR (ctx->r_ptr / r_view / r_cost) and adjacency.  No synchronisation at the end: the
// solver's launches queue behind the set-up on the same stream.
void mrf_setup(mvs_ctx* ctx, const mvs_mrf_params* params) {
    ctx->m_params = *params;
    setup_check_params(params);
    Setup S = setup_edge_count(ctx);
    setup_bitmaps(ctx, S);
    setup_sizes_and_classes(ctx, S);
    setup_colouring(ctx, S);
    setup_schedule_order(ctx, S);
    const uint32_t* in_off = setup_message_layout(ctx, S);
    setup_read_sizes(ctx, S);
    setup_edge_table(ctx, S, in_off);
    setup_fast_records(ctx, S);
    setup_generic_maps(ctx, S);
    const mvs_mrf_progress init = setup_decode_buffers(ctx, S, params);
    setup_solver_state(ctx, S, params, init);
}

}  // namespace mvs
