// k_jpegdec.hip -- view input: baseline JPEG files decoded on the device into the image buffers rows A - f10 read (DESIGN.md section 4
// "View input"; jpeg_dec.h defines the format accepted and every step of the arithmetic, and holds the host twin).
//   The host reads the markers up to SOS (jpeg_dec.h parse_headers).  The entropy data of a batch of files goes to the device as it
//   lies in the files, through the pinned upload ring, and then:
//     unstuff     flag_kernel marks the 0x00 behind every 0xFF and both bytes of every RSTn, two scans (sort_scan.h) give every kept byte
//                 its place and every marker its number, compact_kernel leaves the clean bytes and the start of every restart segment
//                 and checks the markers' order;
//     synchronise every segment is cut into subsequences of S bytes (option "jpegdec_subseq_bytes"), one lane each, 256 to a workgroup
//                 (a window; windows never span images).  sync_kernel: every lane decodes its subsequence from a guessed state, then
//                 again from its predecessor's exit state until no exit state of the window changes; launched again until no window
//                 changed one.  Every loop is bounded: 256 rounds, (windows + 1) launches;
//     decode      the blocks that end in a subsequence, scanned, give every subsequence its first block; final_kernel decodes once
//                 more from the exact states, writes int16 coefficients (DC differences as they come) and raises the error bits;
//                 a segmented scan over MCUs makes the differences values (dc_kernel);
//     IDCT        idct_kernel, eight lanes per block, one column then one row each, the transpose through LDS;
//     colour      colour_kernel upsamples the chroma planes and writes interleaved RGB in 16-byte stores into the destination image.
//   Scratch is bounded by mvs_jpegdec_params.max_scratch_bytes: the files are decoded in batches that fit (view_batches.h cut_batches).
#include "view_input.h"
#include "image_routes.h"
#include "jpeg_dec.h"
#include "png_dec.h"

namespace mvs {

using namespace jpeg_dec;
typedef unsigned long long u64;

namespace {

constexpr uint32_t THREADS = 256;            // lanes of a window
constexpr uint32_t MAX_ROUNDS = 256;
constexpr uint32_t STATE_EXACT0 = 0u;        // (overshoot 0, slot 0, index 0): a segment's first state, and every lane's first guess
constexpr uint32_t NO_STATE = 0xFFFFFFFFu;

// per image of a batch (host made)
struct ImgDev {
    uint32_t raw_begin, raw_len;   // its entropy data in the batch's raw bytes (raw_begin: a multiple of 16)
    uint32_t seg_first;            // its first restart segment among the batch's; seg_start holds one more entry per image: index seg_first + image + k
    uint32_t blk_first, mcu_first; // its first block / MCU among the batch's
    uint32_t pad_;
    u64 plane[3];                  // its planes in the batch's plane bytes (multiples of 16)
    uint8_t* dst;                  // its RGB image
};
struct ImgInfo { uint32_t err, nsub, stuffed, found; };   // per image, device made
struct Words { uint32_t changed, rounds_max, exact; uint32_t pad_; };

struct Batch {
    const ImgDev* img; const Frame* frame; ImgInfo* info; uint32_t n;
    const uint32_t* seg_ptr;       // [n + 1] restart segments in front of image i (seg_first)
    uint32_t* seg_start;           // clean position of every segment's first byte, and per image its end
    const uint32_t* sub_ptr;       // [segments + 1] subsequences in front of every segment
    uint32_t S;
};

__device__ inline uint32_t pack_state(uint32_t over, uint32_t slot, uint32_t k) { return over | slot << 5 | k << 8; }

// ---- unstuff and split ----
__global__ void __launch_bounds__(THREADS) flag_kernel(Batch B, const uint8_t* __restrict__ raw, uint8_t* __restrict__ keep, uint8_t* __restrict__ mark) {
    const uint32_t i = blockIdx.y, l = blockIdx.x * THREADS + threadIdx.x;
    const ImgDev I = B.img[i];
    if (l >= I.raw_len) return;
    const uint8_t* r = raw + I.raw_begin;
    const uint32_t b = r[l], prev = l ? r[l - 1u] : 0u, next = l + 1u < I.raw_len ? r[l + 1u] : 0xFFu;
    uint32_t k = 1, m = 0;
    if (b == 0xFFu) {
        if (next >= 0xD0u && next <= 0xD7u) k = 0;
        else if (next != 0x00u) { k = 0; atomicOr(&B.info[i].err, next == 0xDAu ? E_SECOND_SCAN : next == 0xDCu ? E_DNL : E_MARKER); }
    } else if (prev == 0xFFu) {
        k = 0;
        if (b == 0x00u) atomicAdd(&B.info[i].stuffed, 1u);
        else if (b >= 0xD0u && b <= 0xD7u) m = 1;
    }
    keep[I.raw_begin + l] = (uint8_t)k; mark[I.raw_begin + l] = (uint8_t)m;
}
// pos / mpos: exclusive scans of keep / mark over the batch's raw bytes, one entry more than bytes
__global__ void __launch_bounds__(THREADS) compact_kernel(Batch B, const uint8_t* __restrict__ raw, const uint8_t* __restrict__ keep, const uint8_t* __restrict__ mark,
                                                          const uint32_t* __restrict__ pos, const uint32_t* __restrict__ mpos, uint8_t* __restrict__ clean) {
    const uint32_t i = blockIdx.y, l = blockIdx.x * THREADS + threadIdx.x;
    const ImgDev I = B.img[i];
    const uint32_t nseg = B.seg_ptr[i + 1u] - B.seg_ptr[i], s0 = I.seg_first + i;
    if (l == 0u) {
        const uint32_t found = mpos[I.raw_begin + I.raw_len] - mpos[I.raw_begin] + 1u;
        B.seg_start[s0] = pos[I.raw_begin]; B.seg_start[s0 + nseg] = pos[I.raw_begin + I.raw_len];
        B.info[i].found = found;
        if (found != nseg) atomicOr(&B.info[i].err, E_SEGMENTS);
    }
    if (l >= I.raw_len) return;
    const uint32_t g = I.raw_begin + l;
    if (keep[g]) clean[pos[g]] = raw[g];
    if (mark[g]) {
        const uint32_t m = mpos[g] - mpos[I.raw_begin];   // markers in front of this one
        if (raw[g] != 0xD0u + (m & 7u)) atomicOr(&B.info[i].err, E_RST_ORDER);
        if (m + 1u < nseg) B.seg_start[s0 + m + 1u] = pos[g];
    }
}
// subsequences of every segment (at least one); an image already refused counts one per segment: its table may be incomplete
__global__ void __launch_bounds__(THREADS) nsub_kernel(Batch B, uint32_t n_seg, uint32_t* __restrict__ nsub) {
    const uint32_t g = blockIdx.x * THREADS + threadIdx.x;
    if (g >= n_seg) return;
    const uint32_t i = owner_of(B.seg_ptr, B.n, g), e = B.img[i].seg_first + i + (g - B.seg_ptr[i]);
    const uint32_t len = B.seg_start[e + 1u] - B.seg_start[e];
    nsub[g] = B.info[i].err ? 1u : max(1u, (len + B.S - 1u) / B.S);
}
__global__ void __launch_bounds__(THREADS) info_kernel(Batch B) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i < B.n) B.info[i].nsub = B.sub_ptr[B.seg_ptr[i + 1u]] - B.sub_ptr[B.seg_ptr[i]];
}

// ---- a window: 256 consecutive subsequences of one image, their bytes and the image's tables in LDS ----
// LDS bytes are padded by one word per 128 so that lanes 128 bytes apart read different banks
__device__ inline uint32_t lds_at(uint32_t a) { return a + ((a >> 7) << 2); }
// a window's LDS, all of it dynamic: the frame, the lanes' exit states, the window's clean range, the bytes
constexpr uint32_t LDS_STATES = (sizeof(Frame) + 15u) / 16u * 16u, LDS_RANGE = LDS_STATES + THREADS * 4u, LDS_BYTES = LDS_RANGE + 16u;
constexpr uint32_t window_lds_bytes(uint32_t S) { return LDS_BYTES + ((THREADS * S + 64u) / 128u + 1u) * 132u; }

struct Lane {
    bool valid; uint32_t image, sub, seg_entry, seg_k, j, n_in_seg;   // sub: among the batch's; seg_entry: index into seg_start; j: place in the segment
    uint32_t seg_begin, seg_len;                                     // clean bytes of the segment
    uint32_t begin_bit, end_bit;                                     // of the subsequence, inside the segment
};
struct Window {
    const Frame* F; const uint32_t* bytes; uint32_t base;            // LDS; base: clean position of LDS byte 0
};
// every lane's subsequence, and the window's bytes staged (ends with a barrier)
__device__ inline Lane open_window(const Batch& B, const uint32_t* __restrict__ win_ptr, const uint8_t* __restrict__ clean, char* smem, Window& W) {
    uint32_t* range = reinterpret_cast<uint32_t*>(smem + LDS_RANGE);
    const uint32_t tid = threadIdx.x, i = owner_of(win_ptr, B.n, blockIdx.x), w = blockIdx.x - win_ptr[i];
    const uint32_t sA = B.seg_ptr[i], sB = B.seg_ptr[i + 1u], sub0 = B.sub_ptr[sA], subs = B.sub_ptr[sB] - sub0;
    Lane L{};
    L.image = i; L.sub = sub0 + w * THREADS + tid; L.valid = w * THREADS + tid < subs;
    if (L.valid) {
        uint32_t lo = sA, hi = sB;   // the segment with sub_ptr[s] <= sub < sub_ptr[s + 1]
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (B.sub_ptr[mid] <= L.sub) lo = mid; else hi = mid; }
        L.seg_k = lo - sA; L.seg_entry = B.img[i].seg_first + i + L.seg_k; L.j = L.sub - B.sub_ptr[lo]; L.n_in_seg = B.sub_ptr[lo + 1u] - B.sub_ptr[lo];
        L.seg_begin = B.seg_start[L.seg_entry]; L.seg_len = B.seg_start[L.seg_entry + 1u] - L.seg_begin;
        L.begin_bit = min(L.j * B.S, L.seg_len) * 8u; L.end_bit = min((L.j + 1u) * B.S, L.seg_len) * 8u;
    }
    const uint32_t n_valid = min(THREADS, subs - w * THREADS);
    if (tid == 0u) range[0] = L.seg_begin + L.begin_bit / 8u;
    if (tid == n_valid - 1u) range[1] = L.seg_begin + L.end_bit / 8u;
    Frame* F = reinterpret_cast<Frame*>(smem);
    uint32_t* bytes = reinterpret_cast<uint32_t*>(smem + LDS_BYTES);
    for (uint32_t k = tid; k < sizeof(Frame) / 4u; k += THREADS) reinterpret_cast<uint32_t*>(F)[k] = reinterpret_cast<const uint32_t*>(B.frame + i)[k];
    __syncthreads();
    const uint32_t base = range[0] & ~15u, chunks = min((range[1] + 8u - base + 15u) / 16u, (THREADS * B.S + 64u) / 16u);
    for (uint32_t c = tid; c < chunks; c += THREADS) {   // (the clean bytes have 64 bytes of room behind them)
        const uint4 v = *reinterpret_cast<const uint4*>(clean + base + 16u * c);
        uint32_t* d = bytes + lds_at(16u * c) / 4u;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    W.F = F; W.bytes = bytes; W.base = base;
    return L;
}
// byte i of the lane's segment, 0 behind its end
struct SegBytes {
    const uint32_t* bytes; uint32_t off, len;   // off: the segment's first byte in the LDS bytes
    __device__ uint32_t operator()(uint32_t i) const {
        if (i >= len) return 0u;
        const uint32_t a = lds_at(off + i);
        return (bytes[a >> 2] >> (8u * (a & 3u))) & 0xFFu;
    }
};
// the lane's subsequence from the exit state `entry` of its predecessor: its own exit state and the blocks that end in it
__device__ inline uint32_t run_subsequence(const Window& W, const Lane& L, uint32_t entry, uint32_t& blocks) {
    const SegBytes by{W.bytes, L.seg_begin - W.base, L.seg_len};
    State s{L.begin_bit + (entry & 31u), min((entry >> 5) & 7u, W.F->bpm - 1u), min(entry >> 8, 63u)};
    blocks = 0;
    while (s.pos < L.end_bit) blocks += step(*W.F, by, s).block_done ? 1u : 0u;
    return pack_state(min(s.pos - L.end_bit, 31u), s.slot, s.k);
}

// state / entry / cnt: per subsequence its exit state, the entry state that gave it, the blocks that end in it; state1: the first guess's exit state
__global__ void __launch_bounds__(THREADS) sync_kernel(Batch B, const uint32_t* __restrict__ win_ptr, const uint8_t* __restrict__ clean, uint32_t first,
                                                       uint32_t* state, uint32_t* __restrict__ entry, uint32_t* __restrict__ cnt, uint32_t* __restrict__ state1, Words* words) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* st = reinterpret_cast<uint32_t*>(smem + LDS_STATES);
    Window W;
    const Lane L = open_window(B, win_ptr, clean, smem, W);
    const uint32_t tid = threadIdx.x;
    uint32_t mine = NO_STATE, used = NO_STATE, blocks = 0;
    bool window_changed = false;
    if (L.valid) {
        if (first) {
            used = STATE_EXACT0; mine = run_subsequence(W, L, used, blocks);
            state1[L.sub] = mine;
            window_changed = L.j != 0u && tid == 0u && blockIdx.x != win_ptr[L.image];   // its first lane guessed and has a predecessor in another window
        } else { mine = state[L.sub]; used = entry[L.sub]; blocks = cnt[L.sub]; }
    }
    // the exit state in front of the window: another window's, as it is now (a word: never torn); a later launch sees what it became
    const uint32_t outside = !first && L.valid && tid == 0u && L.j != 0u ? __hip_atomic_load(state + L.sub - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : STATE_EXACT0;
    st[tid] = mine;
    uint32_t rounds = 0;
    for (; rounds < MAX_ROUNDS; ++rounds) {
        __syncthreads();
        bool changed = false;
        uint32_t next = mine;
        if (L.valid) {
            const uint32_t pred = L.j == 0u ? STATE_EXACT0 : tid == 0u ? outside : st[tid - 1u];
            if (pred != used) { used = pred; next = run_subsequence(W, L, pred, blocks); changed = next != mine; }
        }
        __syncthreads();
        if (changed) { mine = next; st[tid] = mine; }
        if (!__syncthreads_or(changed ? 1 : 0)) { ++rounds; break; }   // (the round that found nothing to do counts)
        window_changed = true;
    }
    if (L.valid) { __hip_atomic_store(state + L.sub, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); entry[L.sub] = used; cnt[L.sub] = blocks; }
    if (tid == 0u) { if (window_changed) atomicOr(&words->changed, 1u); atomicMax(&words->rounds_max, rounds); }
}

// blk_sub: exclusive scan of cnt over the batch's subsequences
__global__ void __launch_bounds__(THREADS) final_kernel(Batch B, const uint32_t* __restrict__ win_ptr, const uint8_t* __restrict__ clean, const uint32_t* __restrict__ state,
                                                        const uint32_t* __restrict__ state1, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ blk_sub,
                                                        int16_t* __restrict__ coef, Words* words) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Window W;
    const Lane L = open_window(B, win_ptr, clean, smem, W);
    if (!L.valid) return;
    const Frame& F = *W.F;
    const uint32_t mcus = F.mw * F.mh, m0 = L.seg_k * F.interval, due = min(F.interval, mcus - m0) * F.bpm;
    const uint32_t seg_sub0 = L.sub - L.j;
    uint32_t local = blk_sub[L.sub] - blk_sub[seg_sub0], err = 0;   // the block of the segment this lane starts in
    if (state1[L.sub] == state[L.sub]) atomicAdd(&words->exact, 1u);
    if (L.j + 1u == L.n_in_seg && local + cnt[L.sub] < due) err |= E_INCOMPLETE;
    const uint32_t e = L.j ? state[L.sub - 1u] : STATE_EXACT0;
    const SegBytes by{W.bytes, L.seg_begin - W.base, L.seg_len};
    State s{L.begin_bit + (e & 31u), min((e >> 5) & 7u, F.bpm - 1u), min(e >> 8, 63u)};
    int16_t* out = coef + ((u64)B.img[L.image].blk_first + (u64)m0 * F.bpm) * 64u;
    while (s.pos < L.end_bit && local < due) {
        const Step r = step(F, by, s);
        if (r.err) { err |= r.err; break; }
        if (s.pos > 8u * L.seg_len) { err |= E_INCOMPLETE; break; }
        if (r.zz >= 0) out[(u64)local * 64u + F.zz[r.zz]] = (int16_t)r.value;
        if (r.block_done) ++local;
    }
    if (err) atomicOr(&B.info[L.image].err, err);
}

// ---- DC differences -> values: per MCU the sums of its differences, a scan that restarts at every segment, the values written back ----
struct McuSum { int32_t c[3]; uint32_t restart; };
struct McuAdd {
    __host__ __device__ McuSum operator()(const McuSum& a, const McuSum& b) const {
        if (b.restart) return b;
        return McuSum{{a.c[0] + b.c[0], a.c[1] + b.c[1], a.c[2] + b.c[2]}, a.restart};
    }
};
__global__ void __launch_bounds__(THREADS) mcu_sum_kernel(Batch B, const uint32_t* __restrict__ mcu_ptr, uint32_t n_mcu, const int16_t* __restrict__ coef, McuSum* __restrict__ sums) {
    const uint32_t g = blockIdx.x * THREADS + threadIdx.x;
    if (g >= n_mcu) return;
    const uint32_t i = owner_of(mcu_ptr, B.n, g), m = g - mcu_ptr[i];
    const Frame& F = B.frame[i];
    const int16_t* c = coef + ((u64)B.img[i].blk_first + (u64)m * F.bpm) * 64u;
    McuSum s{{0, 0, 0}, m % F.interval == 0u ? 1u : 0u};
    for (uint32_t slot = 0; slot < F.bpm; ++slot) s.c[slot_comp(F, slot)] += c[64u * slot];
    sums[g] = s;
}
__global__ void __launch_bounds__(THREADS) dc_kernel(Batch B, const uint32_t* __restrict__ mcu_ptr, uint32_t n_mcu, int16_t* __restrict__ coef, const McuSum* __restrict__ sums,
                                                     const McuSum* __restrict__ scanned) {
    const uint32_t g = blockIdx.x * THREADS + threadIdx.x;
    if (g >= n_mcu) return;
    const uint32_t i = owner_of(mcu_ptr, B.n, g), m = g - mcu_ptr[i];
    const Frame& F = B.frame[i];
    int16_t* c = coef + ((u64)B.img[i].blk_first + (u64)m * F.bpm) * 64u;
    int32_t pred[3]; bool bad = false;
    for (int k = 0; k < 3; ++k) pred[k] = scanned[g].c[k] - sums[g].c[k];   // (inclusive: a restarting MCU's is its own sum)
    for (uint32_t slot = 0; slot < F.bpm; ++slot) {
        int32_t& p = pred[slot_comp(F, slot)];
        p += c[64u * slot];
        bad |= p < -32768 || p > 32767;
        c[64u * slot] = (int16_t)p;
    }
    if (bad) atomicOr(&B.info[i].err, E_DC);
}

// ---- IDCT: eight lanes per block ----
constexpr uint32_t TILE_PITCH = 9, IDCT_BLOCKS = THREADS / 8u;
__global__ void __launch_bounds__(THREADS) idct_kernel(Batch B, const uint32_t* __restrict__ blk_ptr, uint32_t n_blk, const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
    __shared__ int32_t tile[IDCT_BLOCKS * 8u * TILE_PITCH];
    const uint32_t tid = threadIdx.x, lb = tid >> 3, lane = tid & 7u, g = blockIdx.x * IDCT_BLOCKS + lb;
    const bool live = g < n_blk;
    uint32_t i = 0, c = 0, x0 = 0, y0 = 0; bool f32 = true;
    if (live) {
        i = owner_of(blk_ptr, B.n, g);
        const Frame& F = B.frame[i];
        block_place(F, g - blk_ptr[i], c, x0, y0);
        int32_t in[8], out[8], sum = 0;
        for (uint32_t y = 0; y < 8u; ++y) { in[y] = (int32_t)coef[(u64)g * 64u + 8u * y + lane] * (int32_t)F.quant[c][8u * y + lane]; sum += min(abs(in[y]), IDCT_FITS32 + 1); }
        for (int d = 1; d < 8; d <<= 1) sum += __shfl_xor(sum, d);   // (at most 64 x 5401: no overflow; the eight lanes of a block are neighbours in a wave)
        f32 = idct_fits32(sum);
        idct_column(in, out, f32);
        for (uint32_t y = 0; y < 8u; ++y) tile[(lb * 8u + y) * TILE_PITCH + lane] = out[y];
    }
    __syncthreads();
    if (!live) return;
    const Frame& F = B.frame[i];
    int32_t in[8];
    for (uint32_t x = 0; x < 8u; ++x) in[x] = tile[(lb * 8u + lane) * TILE_PITCH + x];
    union { uint8_t b[8]; uint2 w; } o;
    idct_row(in, o.b, f32);
    *reinterpret_cast<uint2*>(planes + B.img[i].plane[c] + (u64)(y0 + lane) * plane_pitch(F, c) + x0) = o.w;
}

// ---- upsampling and colour: a lane makes 16 bytes of the destination, aligned to it ----
__global__ void __launch_bounds__(THREADS) colour_kernel(Batch B, const u64* __restrict__ chunk_ptr, u64 n_chunks, const uint8_t* __restrict__ planes) {
    const u64 g = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n_chunks) return;
    const uint32_t i = span_of(chunk_ptr, B.n, g);
    const Frame& F = B.frame[i];
    const ImgDev& I = B.img[i];
    const u64 bytes = 3ull * F.width * F.height, lead = (u64)((uintptr_t)I.dst & 15u), q = g - chunk_ptr[i];
    const u64 t0 = q * 16u < lead ? 0ull : q * 16u - lead, t1 = min(bytes, (q + 1u) * 16u - lead);   // the image's bytes [t0, t1) of this chunk
    const uint8_t* py = planes + I.plane[0]; const uint8_t* pb = planes + I.plane[1]; const uint8_t* pr = planes + I.plane[2];
    const uint32_t pitch_y = plane_pitch(F, 0), pitch_c = plane_pitch(F, 1);
    union { uint8_t b[16]; uint4 w; } o;
    for (u64 p = t0 / 3u; p * 3u < t1; ++p) {
        const uint32_t x = (uint32_t)(p % F.width), y = (uint32_t)(p / F.width);
        uint8_t rgb[3];
        const int32_t Y = py[(u64)y * pitch_y + x];
        if (F.ncomp == 1u) rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
        else {
            auto cb = [&](uint32_t a, uint32_t b) -> int32_t { return pb[(u64)b * pitch_c + a]; };
            auto cr = [&](uint32_t a, uint32_t b) -> int32_t { return pr[(u64)b * pitch_c + a]; };
            colour(Y, upsampled(cb, F.cw, F.ch, F.hs, F.vs, x, y), upsampled(cr, F.cw, F.ch, F.hs, F.vs, x, y), rgb);
        }
        for (uint32_t k = 0; k < 3u; ++k) { const u64 t = p * 3u + k; if (t >= t0 && t < t1) o.b[t - t0] = rgb[k]; }
    }
    if (t1 - t0 == 16u) *reinterpret_cast<uint4*>(I.dst + t0) = o.w;
    else for (u64 t = t0; t < t1; ++t) I.dst[t] = o.b[t - t0];
}

}  // namespace

// per-context buffers of the route, allocated on first use
struct JpegDecDev {
    DBuf<uint8_t> raw, keep, mark, clean, planes, out; DBuf<uint32_t> pos, mpos, t32, seg_start, nsub, sub_ptr, state, state1, entry, cnt, blk_sub, words;
    DBuf<ImgDev> img; DBuf<Frame> frame; DBuf<ImgInfo> info; DBuf<int16_t> coef; DBuf<McuSum> sums, scanned; DBuf<u64> t64;
};
void jpegdec_release(mvs_ctx* ctx) { delete ctx->jpegdec; ctx->jpegdec = nullptr; }

namespace {

struct HostFile { Frame F; size_t begin = 0, raw_len = 0; uint64_t scratch = 0; uint32_t view = 0; };   // view: its number in the caller's list

// the scratch one file needs: raw, keep, mark, clean (1 each) and two scans (4 each) per entropy byte, 16 bytes per subsequence,
// 128 bytes of coefficients per block, 32 per MCU, the planes
uint64_t file_scratch(const HostFile& f, uint32_t S) {
    const uint64_t raw = align16(f.raw_len) + 64u, subs = raw / S + f.F.nseg + 1u, mcus = (uint64_t)f.F.mw * f.F.mh, blocks = mcus * f.F.bpm;
    uint64_t planes = 0;
    for (uint32_t c = 0; c < f.F.ncomp; ++c) planes += align16((uint64_t)plane_pitch(f.F, c) * plane_rows(f.F, c));
    return 12u * raw + 16u * subs + 4u * (f.F.nseg + 2u) * 3u + 128u * blocks + 32u * mcus + planes + sizeof(Frame) + sizeof(ImgDev) + sizeof(ImgInfo);
}

// files [a, b) of the call, decoded into dst[a .. b)
void decode_batch(mvs_ctx* ctx, JpegDecDev& D, const uint8_t* const* files, const std::vector<HostFile>& H, uint32_t a, uint32_t b, uint8_t* const* dst, const char* who, mvs_jpegdec_stats& st) {
    hipStream_t s = ctx->stream;
    const uint32_t n = b - a, S = ctx->jpegdec_subseq;
    std::vector<ImgDev> img(n); std::vector<Frame> frame(n);
    std::vector<uint32_t> t32(4 * ((size_t)n + 1));   // seg_ptr, mcu_ptr, blk_ptr, win_ptr: [n + 1] each
    uint32_t* seg_ptr = t32.data(); uint32_t* mcu_ptr = seg_ptr + n + 1; uint32_t* blk_ptr = mcu_ptr + n + 1; uint32_t* win_ptr = blk_ptr + n + 1;
    std::vector<uint64_t> chunks(n);
    uint64_t raw_total = 0, plane_total = 0, seg = 0, mcu = 0, blk = 0; uint32_t raw_max = 0;
    seg_ptr[0] = mcu_ptr[0] = blk_ptr[0] = win_ptr[0] = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const HostFile& f = H[a + k];
        ImgDev& I = img[k];
        frame[k] = f.F;
        I.raw_begin = (uint32_t)raw_total; I.raw_len = (uint32_t)f.raw_len; raw_total += align16(f.raw_len); raw_max = std::max(raw_max, I.raw_len);
        I.seg_first = (uint32_t)seg; I.mcu_first = (uint32_t)mcu; I.blk_first = (uint32_t)blk; I.pad_ = 0;
        seg += f.F.nseg; mcu += (uint64_t)f.F.mw * f.F.mh; blk += (uint64_t)f.F.mw * f.F.mh * f.F.bpm;
        for (uint32_t c = 0; c < 3u; ++c) { I.plane[c] = plane_total; if (c < f.F.ncomp) plane_total += align16((uint64_t)plane_pitch(f.F, c) * plane_rows(f.F, c)); }
        I.dst = dst[a + k];
        const uint64_t bytes = 3ull * f.F.width * f.F.height;
        chunks[k] = (((uintptr_t)I.dst & 15u) + bytes + 15u) / 16u;
        seg_ptr[k + 1] = (uint32_t)seg; mcu_ptr[k + 1] = (uint32_t)mcu; blk_ptr[k + 1] = (uint32_t)blk;
        if (raw_total >= 0x7FFFFFF0ull || blk * 64u >= 0xFFFFFFFFFFull || blk >= 0x7FFFFFFFull || seg + n >= 0x7FFFFFFFull)
            throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": a batch too large for 32-bit positions (lower max_scratch_bytes)");
    }
    const uint32_t N = (uint32_t)raw_total, NSEG = (uint32_t)seg, NMCU = (uint32_t)mcu, NBLK = (uint32_t)blk;
    st.entropy_bytes += [&] { uint64_t v = 0; for (uint32_t k = 0; k < n; ++k) v += img[k].raw_len; return v; }();
    st.restart_segments += NSEG; st.blocks += NBLK; st.batches += 1;

    StageTimer<7> tm(s);
    tm.mark();
    // ---- upload: the entropy data through the pinned ring, the tables ----
    D.raw.ensure((size_t)N + 64); D.keep.ensure((size_t)N + 64); D.mark.ensure((size_t)N + 64); D.clean.ensure((size_t)N + 128);
    D.pos.ensure((size_t)N + 2); D.mpos.ensure((size_t)N + 2);
    D.seg_start.ensure((size_t)NSEG + n + 1); D.nsub.ensure((size_t)NSEG + 2); D.sub_ptr.ensure((size_t)NSEG + 2); D.info.ensure(n); D.words.ensure(4);
    D.coef.ensure((size_t)NBLK * 64 + 64); D.sums.ensure((size_t)NMCU + 1); D.scanned.ensure((size_t)NMCU + 1); D.planes.ensure((size_t)plane_total + 16);
    MVS_HIP(hipMemsetAsync(D.raw.p, 0, (size_t)N + 64, s));
    MVS_HIP(hipMemsetAsync(D.keep.p, 0, (size_t)N + 64, s)); MVS_HIP(hipMemsetAsync(D.mark.p, 0, (size_t)N + 64, s));
    MVS_HIP(hipMemsetAsync(D.clean.p, 0, (size_t)N + 128, s));
    MVS_HIP(hipMemsetAsync(D.info.p, 0, n * sizeof(ImgInfo), s)); MVS_HIP(hipMemsetAsync(D.words.p, 0, sizeof(Words), s));
    MVS_HIP(hipMemsetAsync(D.seg_start.p, 0, ((size_t)NSEG + n + 1) * sizeof(uint32_t), s));
    MVS_HIP(hipMemsetAsync(D.coef.p, 0, ((size_t)NBLK * 64 + 64) * sizeof(int16_t), s));
    upload(D.img, img, s); upload(D.frame, frame, s); upload(D.t32, t32, s);
    {
        std::vector<const uint8_t*> src(n); std::vector<uint8_t*> to(n); std::vector<size_t> nb(n);
        for (uint32_t k = 0; k < n; ++k) { src[k] = files[a + k] + H[a + k].begin; to[k] = D.raw.p + img[k].raw_begin; nb[k] = img[k].raw_len; }
        upload_pieces_through_ring(ctx, src.data(), to.data(), nb.data(), n);
    }
    MVS_HIP(hipStreamSynchronize(s));   // (img, frame and t32 are this function's: they stay alive, but win_ptr is written again below)
    tm.mark();
    // ---- unstuff and split ----
    Batch B{D.img.p, D.frame.p, D.info.p, n, D.t32.p, D.seg_start.p, D.sub_ptr.p, S};
    const dim3 byte_grid(grid(raw_max), n);
    hipLaunchKernelGGL(flag_kernel, byte_grid, dim3(THREADS), 0, s, B, (const uint8_t*)D.raw.p, D.keep.p, D.mark.p);
    MVS_LAUNCH_CHECK();
    dev_exclusive_scan(ctx, (const uint8_t*)D.keep.p, D.pos.p, (size_t)N + 1);
    dev_exclusive_scan(ctx, (const uint8_t*)D.mark.p, D.mpos.p, (size_t)N + 1);
    hipLaunchKernelGGL(compact_kernel, byte_grid, dim3(THREADS), 0, s, B, (const uint8_t*)D.raw.p, (const uint8_t*)D.keep.p, (const uint8_t*)D.mark.p,
                       (const uint32_t*)D.pos.p, (const uint32_t*)D.mpos.p, D.clean.p);
    MVS_LAUNCH_CHECK();
    hipLaunchKernelGGL(nsub_kernel, dim3(grid(NSEG)), dim3(THREADS), 0, s, B, NSEG, D.nsub.p);
    MVS_LAUNCH_CHECK();
    MVS_HIP(hipMemsetAsync(D.nsub.p + NSEG, 0, sizeof(uint32_t), s));
    dev_exclusive_scan(ctx, (const uint32_t*)D.nsub.p, D.sub_ptr.p, (size_t)NSEG + 1);
    hipLaunchKernelGGL(info_kernel, dim3(grid(n)), dim3(THREADS), 0, s, B);
    MVS_LAUNCH_CHECK();
    std::vector<ImgInfo> info(n);
    auto read_info = [&] {
        ctx->row_pin.ensure(n * sizeof(ImgInfo));
        MVS_HIP(hipMemcpyAsync(ctx->row_pin.p, D.info.p, n * sizeof(ImgInfo), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));
        memcpy(info.data(), ctx->row_pin.p, n * sizeof(ImgInfo));
        for (uint32_t k = 0; k < n; ++k)
            if (info[k].err) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(H[a + k].view) + ": jpeg: " + err_text(info[k].err));
    };
    tm.mark();
    uint64_t nsub_total = 0, nwin = 0, win_longest = 0;
    try { read_info(); } catch (...) { for (uint32_t k = 0; k < n; ++k) st.stuffed_bytes += info[k].stuffed; st.ms_upload += tm.ms(0, 1); st.ms_unstuff += tm.ms(1, 2); throw; }
    for (uint32_t k = 0; k < n; ++k) {
        st.stuffed_bytes += info[k].stuffed; nsub_total += info[k].nsub;
        const uint64_t w = (info[k].nsub + THREADS - 1u) / THREADS;
        nwin += w; win_longest = std::max(win_longest, w); win_ptr[k + 1] = (uint32_t)nwin;
    }
    if (nwin >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": too many windows in one batch");
    st.subsequences += nsub_total; st.windows += nwin;
    const uint32_t NSUB = (uint32_t)nsub_total, NWIN = (uint32_t)nwin;
    MVS_HIP(hipMemcpyAsync(D.t32.p + 3 * ((size_t)n + 1), win_ptr, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    const uint32_t* d_win = D.t32.p + 3 * ((size_t)n + 1);
    D.state.ensure((size_t)NSUB + 1); D.state1.ensure((size_t)NSUB + 1); D.entry.ensure((size_t)NSUB + 1); D.cnt.ensure((size_t)NSUB + 2); D.blk_sub.ensure((size_t)NSUB + 2);
    // ---- synchronise ----
    const uint32_t lds = window_lds_bytes(S);
    Words* words = reinterpret_cast<Words*>(D.words.p);
    uint32_t launches = 0;
    for (;; ++launches) {
        if (launches > win_longest + 1u) throw StatusError(MVS_ERR_INVALID, std::string(who) + ": the subsequences did not synchronise within their bound");
        MVS_HIP(hipMemsetAsync(&words->changed, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(sync_kernel, dim3(NWIN), dim3(THREADS), lds, s, B, d_win, (const uint8_t*)D.clean.p, launches == 0u ? 1u : 0u, D.state.p, D.entry.p, D.cnt.p, D.state1.p, words);
        MVS_LAUNCH_CHECK();
        if (!read_word(ctx, &words->changed)) { ++launches; break; }
    }
    st.sync_launches += launches;
    tm.mark();
    // ---- decode ----
    MVS_HIP(hipMemsetAsync(D.cnt.p + NSUB, 0, sizeof(uint32_t), s));
    dev_exclusive_scan(ctx, (const uint32_t*)D.cnt.p, D.blk_sub.p, (size_t)NSUB + 1);
    hipLaunchKernelGGL(final_kernel, dim3(NWIN), dim3(THREADS), lds, s, B, d_win, (const uint8_t*)D.clean.p, (const uint32_t*)D.state.p, (const uint32_t*)D.state1.p,
                       (const uint32_t*)D.cnt.p, (const uint32_t*)D.blk_sub.p, D.coef.p, words);
    MVS_LAUNCH_CHECK();
    const uint32_t* d_mcu = D.t32.p + ((size_t)n + 1); const uint32_t* d_blk = D.t32.p + 2 * ((size_t)n + 1);
    hipLaunchKernelGGL(mcu_sum_kernel, dim3(grid(NMCU)), dim3(THREADS), 0, s, B, d_mcu, NMCU, (const int16_t*)D.coef.p, D.sums.p);
    MVS_LAUNCH_CHECK();
    with_sort_tmp(ctx, [&](void* t, size_t& bytes) { return rocprim::inclusive_scan(t, bytes, D.sums.p, D.scanned.p, (size_t)NMCU, McuAdd(), s); });
    hipLaunchKernelGGL(dc_kernel, dim3(grid(NMCU)), dim3(THREADS), 0, s, B, d_mcu, NMCU, D.coef.p, (const McuSum*)D.sums.p, (const McuSum*)D.scanned.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    // ---- IDCT ----
    hipLaunchKernelGGL(idct_kernel, dim3((NBLK + IDCT_BLOCKS - 1u) / IDCT_BLOCKS), dim3(THREADS), 0, s, B, d_blk, NBLK, (const int16_t*)D.coef.p, D.planes.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    // ---- upsampling and colour ----
    const std::vector<u64> chunk_ptr = span_prefix(chunks);
    upload(D.t64, chunk_ptr, s);
    const u64 n_chunks = chunk_ptr[n];
    uint64_t colour_blocks = 0;
    if (!span_blocks(n_chunks, THREADS, true, colour_blocks)) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": too many pixels in one batch");
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)colour_blocks), dim3(THREADS), 0, s, B, (const u64*)D.t64.p, n_chunks, (const uint8_t*)D.planes.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    uint32_t hw[4];
    read_words(ctx, words, hw, 4);
    st.sync_rounds_max = std::max<uint64_t>(st.sync_rounds_max, hw[1]); st.subseq_exact_after_pass1 += hw[2];
    st.ms_upload += tm.ms(0, 1); st.ms_unstuff += tm.ms(1, 2); st.ms_sync += tm.ms(2, 3); st.ms_decode += tm.ms(3, 4); st.ms_idct += tm.ms(4, 5); st.ms_colour += tm.ms(5, 6);
    read_info();   // (drains the stream: the vectors above were read by asynchronous copies)
}

mvs_jpegdec_params jpegdec_params(const mvs_jpegdec_params* p) { mvs_jpegdec_params P; if (p) P = *p; else mvs_jpegdec_default_params(&P); return P; }

// the headers of all files on the host (file k is view view_no[k] of the caller's list; null: view k); with `views`, a frame must have its view's size
std::vector<HostFile> read_headers(mvs_ctx* ctx, const uint8_t* const* files, const uint64_t* sizes, uint32_t n, const uint32_t* view_no, const mvs_view* views, const char* who, mvs_jpegdec_stats& st) {
    std::vector<HostFile> H(n);
    for (uint32_t k = 0; k < n; ++k) {
        H[k].view = view_no ? view_no[k] : k;
        const std::string w = std::string(who) + ": view " + std::to_string(H[k].view) + ": ";
        if (!files[k]) throw StatusError(MVS_ERR_INVALID, w + "null file");
        std::string msg;
        if (parse_headers(files[k], (size_t)sizes[k], H[k].F, H[k].begin, msg) != MVS_OK) throw StatusError(MVS_ERR_INVALID, w + msg);
        H[k].raw_len = (size_t)sizes[k] - 2 - H[k].begin;
        if (views && ((int64_t)H[k].F.width != views[H[k].view].width || (int64_t)H[k].F.height != views[H[k].view].height))
            throw StatusError(MVS_ERR_INVALID, w + "jpeg: the frame is " + std::to_string(H[k].F.width) + " x " + std::to_string(H[k].F.height) + ", the view " +
                                                   std::to_string(views[H[k].view].width) + " x " + std::to_string(views[H[k].view].height));
        H[k].scratch = file_scratch(H[k], ctx->jpegdec_subseq);
        st.files += 1; st.file_bytes += sizes[k];
    }
    return H;
}
// the batch cut: files [cut[k], cut[k + 1]) are batch k, the longest run whose scratch fits; a file that does not fit alone is refused
std::vector<size_t> cut_files(const std::vector<HostFile>& H, const mvs_jpegdec_params& P, const char* who) {
    std::vector<uint64_t> need(H.size()); std::vector<uint32_t> view(H.size());
    for (size_t k = 0; k < H.size(); ++k) { need[k] = H[k].scratch; view[k] = H[k].view; }
    refuse_over_cap(need, P.max_scratch_bytes, view.data(), who, "scratch");
    return cut_batches(need.data(), need.size(), P.max_scratch_bytes, VIEW_FILES_PER_BATCH);
}

}  // namespace

// the file views of a scene, some of them through the staging (ctx.h)
void decode_view_files(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const uint8_t* const* files, const uint64_t* sizes, uint8_t* const* dst, const uint8_t* staged,
                       const mvs_jpegdec_params* params, const char* who, mvs_jpegdec_stats& st, const StagedBatchFn& after_batch, mvs_pngdec_stats* png_stats) {
    const mvs_jpegdec_params P = jpegdec_params(params);
    FileViews fv = file_views(files, sizes, n_views);
    if (png_stats) {   // the files with the PNG signature leave the list for their own route
        FileViews jpegs, pngs;
        for (size_t k = 0; k < fv.files.size(); ++k) {
            FileViews& to = png_dec::has_signature(fv.files[k], (size_t)fv.sizes[k]) ? pngs : jpegs;
            to.files.push_back(fv.files[k]); to.sizes.push_back(fv.sizes[k]); to.view.push_back(fv.view[k]);
        }
        if (!pngs.files.empty()) decode_view_pngs(ctx, views, pngs, dst, staged, params, who, *png_stats, after_batch);
        fv = jpegs;
        if (fv.files.empty()) return;
    }
    std::vector<HostFile> H = read_headers(ctx, fv.files.data(), fv.sizes.data(), (uint32_t)fv.files.size(), fv.view.data(), views, who, st);
    const size_t n = H.size();
    std::vector<uint64_t> stage_bytes(n);   // a staged file's decoded pixels count towards its scratch
    for (size_t k = 0; k < n; ++k) { stage_bytes[k] = staged[H[k].view] ? 3ull * H[k].F.width * H[k].F.height : 0ull; H[k].scratch += align16(stage_bytes[k]); }
    const std::vector<size_t> cut = cut_files(H, P, who);
    const BatchLayout L = batch_layout(stage_bytes.data(), n, cut);   // every batch stages from the buffer's start: it is as large as the largest batch needs
    uint8_t* staging = L.most ? view_staging(ctx, L.most) : nullptr;
    std::vector<uint8_t*> to(n);
    for (size_t k = 0; k < n; ++k) to[k] = staged[H[k].view] ? staging + L.off[k] : dst[H[k].view];
    JpegDecDev& D = row_dev(ctx->jpegdec);
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        decode_batch(ctx, D, fv.files.data(), H, (uint32_t)cut[b], (uint32_t)cut[b + 1], to.data(), who, st);
        std::vector<uint32_t> bv; std::vector<const uint8_t*> bp;
        for (size_t k = cut[b]; k < cut[b + 1]; ++k) if (staged[H[k].view]) { bv.push_back(H[k].view); bp.push_back(to[k]); }
        if (!bv.empty()) after_batch(bv, bp);
    }
}

}  // namespace mvs

using namespace mvs;

extern "C" {

void mvs_jpegdec_default_params(mvs_jpegdec_params* p) { if (p) { p->max_scratch_bytes = VIEW_SCRATCH_DEFAULT; p->reserved = 0; } }

mvs_status mvs_ctx_decode_jpegs(mvs_ctx* ctx, const uint8_t* const* files, const uint64_t* sizes, uint32_t n, const mvs_jpegdec_params* params, int out_on_device,
                                mvs_rgb_set* out, mvs_jpegdec_stats* stats) {
    if (!ctx || !out || (n && (!files || !sizes))) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_rgb_set{};
    mvs_jpegdec_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        const mvs_jpegdec_params P = jpegdec_params(params);
        run_with_stats(ctx->stream, stats, st, [&] {
            const std::vector<HostFile> H = read_headers(ctx, files, sizes, n, nullptr, nullptr, "decode_jpegs", st);
            JpegDecDev& D = row_dev(ctx->jpegdec);
            std::vector<uint32_t> w(n), h(n);
            for (uint32_t k = 0; k < n; ++k) { w[k] = H[k].F.width; h[k] = H[k].F.height; }
            const RgbRoom R = rgb_set_room(D.out, w, h);
            const std::vector<size_t> cut = cut_files(H, P, "decode_jpegs");   // all files in batches whose scratch fits
            for (size_t k = 0; k + 1 < cut.size(); ++k) decode_batch(ctx, D, files, H, (uint32_t)cut[k], (uint32_t)cut[k + 1], R.dst.data(), "decode_jpegs", st);
            rgb_set_out(ctx, D.out, R, w, h, out_on_device, out);
        });
    });
}

void mvs_rgb_set_free(mvs_rgb_set* p) {
    if (!p) return;
    if (!p->on_device) free(p->data);
    free(p->offsets); free(p->width); free(p->height);
    *p = mvs_rgb_set{};
}

mvs_status mvs_scene_set_views_jpeg(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const uint8_t* const* files, const uint64_t* sizes, const mvs_jpegdec_params* params,
                                    mvs_jpegdec_stats* stats) {
    if (!ctx || (n_views && (!views || !files || !sizes))) return api_fail(MVS_ERR_INVALID, "null argument");
    return set_views_files(ctx, views, n_views, nullptr, files, sizes, params, stats, nullptr, "", "set_views_jpeg");
}

mvs_status mvs_jpeg_probe(const uint8_t* data, uint64_t size, uint32_t* width, uint32_t* height) {
    if (!data) return api_fail(MVS_ERR_INVALID, "null argument");
    Frame F; size_t begin = 0; std::string msg;
    if (parse_headers(data, (size_t)size, F, begin, msg) != MVS_OK) return api_fail(MVS_ERR_INVALID, msg);
    if (width) *width = F.width;
    if (height) *height = F.height;
    return MVS_OK;
}

mvs_status mvs_decode_jpeg(const uint8_t* data, uint64_t size, uint8_t** rgb, uint32_t* width, uint32_t* height, int16_t** coefs, uint64_t* n_blocks) {
    if (!data || !rgb || !width || !height || (coefs && !n_blocks)) return api_fail(MVS_ERR_INVALID, "null argument");
    *rgb = nullptr; *width = *height = 0;
    if (coefs) { *coefs = nullptr; *n_blocks = 0; }
    std::vector<uint8_t> v; std::vector<int16_t> c; std::string msg; uint64_t nb = 0;
    const mvs_status st = decode_jpeg(data, (size_t)size, v, *width, *height, coefs ? &c : nullptr, msg);
    if (st == MVS_OK && coefs) {
        *coefs = (int16_t*)malloc(std::max<size_t>(c.size(), 1) * sizeof(int16_t));
        if (!*coefs) return api_fail(MVS_ERR_INVALID, "out of host memory");
        if (!c.empty()) memcpy(*coefs, c.data(), c.size() * sizeof(int16_t));
        *n_blocks = c.size() / 64;
    }
    const mvs_status rc = twin_out(st, msg, v, rgb, &nb);
    if (rc != MVS_OK && coefs) { free(*coefs); *coefs = nullptr; *n_blocks = 0; }
    return rc;
}

}  // extern "C"
