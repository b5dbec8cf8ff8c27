// k_pngdec.hip -- view input: PNG files inflated and unfiltered on the device into the image buffers rows A - f10 read (DESIGN.md section 4
// "View input"; png_dec.h defines the format accepted and every step of the arithmetic, and holds the host twin).
//   The host walks the chunks (png_dec.h parse_container).  The IDAT payloads of a batch of files go to the device piece by piece through
//   the pinned upload ring, so that every file's zlib stream lies there back to back, and then:
//     inflate     png_inflate_kernel, one wave64 per stream: png_dec.h inflate() on an environment whose tables and 32 KiB window live in
//                 LDS.  The symbol loop is wave-uniform; the wave builds the tables and executes the stored and match copies with all lanes;
//     Adler-32    adler_piece_kernel sums pieces of 4096 bytes of the inflated stream in one span launch, adler_fold_kernel joins a file's pieces;
//     unfilter    png_unfilter_kernel, one wave64 per file: the lanes take the 64 rows of a band, each one pixel behind the row above, the
//                 finished pixel goes to the lane below by a wave shuffle; the band's input is staged in LDS in skewed segments of 64 pixels,
//                 its last row is carried to the next band.  The pixels leave as RGB straight into the destination image.
//   Scratch is bounded by mvs_jpegdec_params.max_scratch_bytes: the files are decoded in batches that fit (view_batches.h cut_batches).
#include "view_input.h"
#include "image_routes.h"
#include "png_dec.h"

namespace mvs {

using namespace png_dec;
typedef unsigned long long u64;

namespace {

constexpr uint32_t WAVE = 64, WINDOW = 32768, ADLER_THREADS = 256;
static_assert(UNFILTER_BAND == WAVE && UNFILTER_SEGMENT == WAVE, "the unfilter kernel's band and segment are one wave's lanes");

// per file of a batch (host made)
struct FileDev {
    u64 z_begin, raw_begin;          // its zlib stream in the batch's z bytes, its inflated stream in the batch's raw bytes (multiples of 16)
    uint32_t z_len, raw_need;        // bytes of both
    uint32_t width, height, colour_type, bpp, n_plte, carry_begin;   // carry_begin: its row of carried pixels among the batch's
    uint8_t* dst;                    // its RGB image
    uint8_t plte[768];
};
struct FileInfo { uint32_t err, pos, blocks[3], rows[5], adler, produced_lo, produced_hi, pad_; };   // per file, device made
struct AdlerItem { u64 raw_begin; uint32_t need, file; };

__device__ inline void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }   // (the LDS executes a wave's accesses in order: this keeps the compiler from moving them)

struct InflateLds { Huff lit, dist; uint8_t lens[352]; uint16_t nextc[16], offs[16]; uint8_t ring[WINDOW]; };

// png_dec.h inflate()'s environment on one wave: every value it hands out is the same in all lanes
struct DevEnv {
    const uint32_t* words; const uint8_t* zb; uint32_t n, nwords;
    uint8_t* out; uint32_t need; u64 made; InflateLds* S; uint32_t lane;
    template <class T> __device__ T uni(T v) const { return (T)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ uint32_t word(uint32_t i) const { return i < nwords ? uni(words[i]) : 0u; }   // (the stream's slot is zero behind its last byte)
    __device__ uint8_t* lens() { return S->lens; }
    __device__ Huff& lit() { return S->lit; }
    __device__ Huff& dist() { return S->dist; }
    __device__ u64 produced() const { return made; }
    __device__ void store(u64 at, uint32_t b) { S->ring[(uint32_t)at & (WINDOW - 1u)] = (uint8_t)b; if (at < need) out[at] = (uint8_t)b; }
    __device__ void put(uint32_t b) { if (lane == 0u) store(made, b); ++made; }
    __device__ void copy_stored(uint32_t p, uint32_t len) {
        wave_fence();
        for (uint32_t i = lane; i < len; i += WAVE) store(made + i, zb[p + i]);
        made += len;
        wave_fence();
    }
    // dist >= 64: every group of 64 bytes lies in front of what it writes; below, the source is the last `dist` bytes, repeated
    __device__ void copy_match(uint32_t dist, uint32_t len) {
        wave_fence();
        const uint32_t base = (uint32_t)made;
        if (dist >= WAVE) {
            for (uint32_t i = lane; i < len; i += WAVE) { const uint32_t b = S->ring[(base - dist + i) & (WINDOW - 1u)]; store(made + i, b); wave_fence(); }
        } else {
            uint32_t r = lane % dist; const uint32_t m = WAVE % dist;
            for (uint32_t i = lane; i < len; i += WAVE) {
                const uint32_t b = S->ring[(base - dist + r) & (WINDOW - 1u)];
                store(made + i, b);
                r += m; if (r >= dist) r -= dist;
            }
        }
        made += len;
        wave_fence();
    }
    // the table of n <= 288 lengths, built by the wave: a lane per symbol, its place among the codes of its length by ballots
    __device__ uint32_t build(Huff& H, const uint8_t* lens, uint32_t n, uint32_t kind) {
        wave_fence();
        uint32_t cnt[16], my_len[5], my_rank[5];
        for (int l = 0; l < 16; ++l) cnt[l] = 0;
        const u64 below = (1ull << lane) - 1ull;
#pragma unroll
        for (uint32_t c = 0; c < 5u; ++c) {
            const uint32_t s = c * WAVE + lane, l = s < n ? lens[s] : 0u;
            uint32_t rank = 0;
#pragma unroll
            for (uint32_t L = 1; L < 16u; ++L) {
                const u64 m = __ballot(l == L);
                if (l == L) rank = cnt[L] + (uint32_t)__popcll(m & below);
                cnt[L] += (uint32_t)__popcll(m);
            }
            my_len[c] = l; my_rank[c] = rank;
        }
        const uint32_t why = code_refusal(cnt, kind);
        if (why) return why;
        for (uint32_t i = lane; i < (1u << FAST_BITS); i += WAVE) H.look[i] = 0;
        uint32_t code = 0, idx = 0;
#pragma unroll
        for (uint32_t L = 1; L < 16u; ++L) {
            if (lane == 0u) { S->nextc[L] = (uint16_t)code; S->offs[L] = (uint16_t)idx; H.count[L] = (uint16_t)cnt[L]; }
            code = (code + cnt[L]) << 1; idx += cnt[L];
        }
        wave_fence();
#pragma unroll
        for (uint32_t c = 0; c < 5u; ++c) {
            const uint32_t l = my_len[c], s = c * WAVE + lane;
            if (!l) continue;
            H.sym[S->offs[l] + my_rank[c]] = (uint16_t)s;
            if (l <= FAST_BITS) {
                const uint32_t v = S->nextc[l] + my_rank[c];
                for (uint32_t i = __brev(v) >> (32u - l); i < (1u << FAST_BITS); i += 1u << l) H.look[i] = (uint16_t)(l << 9 | s);
            }
        }
        wave_fence();
        return E_NONE;
    }
};

// one wave64 per zlib stream.  Reads nothing outside the stream's slot (its bytes and the zeros up to the next multiple of 16), writes
// nothing outside raw [raw_begin, raw_begin + raw_need).
__global__ void __launch_bounds__(WAVE) png_inflate_kernel(const FileDev* __restrict__ files, FileInfo* __restrict__ info, const uint8_t* __restrict__ z, uint8_t* raw) {
    __shared__ InflateLds S;
    const FileDev& F = files[blockIdx.x];
    DevEnv E{reinterpret_cast<const uint32_t*>(z + F.z_begin), z + F.z_begin, F.z_len, (F.z_len + 3u) / 4u, raw + F.raw_begin, F.raw_need, 0ull, &S, threadIdx.x};
    Inflated R;
    inflate(E, R);
    if (!R.err && R.produced < F.raw_need) { R.err = E_SHORT; R.pos = (uint32_t)R.produced; }
    if (threadIdx.x == 0u) {
        FileInfo& I = info[blockIdx.x];
        I.err = R.err; I.pos = R.pos; I.adler = R.adler; I.produced_lo = (uint32_t)R.produced; I.produced_hi = (uint32_t)(R.produced >> 32);
        for (int k = 0; k < 3; ++k) I.blocks[k] = R.blocks[k];
    }
}

// ---- Adler-32: block g sums one piece of ADLER_PIECE bytes from (1, 0); a thread takes 16 bytes ----
__global__ void __launch_bounds__(ADLER_THREADS) adler_piece_kernel(const AdlerItem* __restrict__ items, uint32_t n, const u64* __restrict__ ptr, const uint8_t* __restrict__ raw, uint2* __restrict__ parts) {
    __shared__ uint32_t red[2 * ADLER_THREADS / WAVE];
    const u64 g = blockIdx.x;
    const uint32_t i = span_of(ptr, n, g), tid = threadIdx.x;
    const AdlerItem I = items[i];
    const uint32_t at = (uint32_t)(g - ptr[i]) * ADLER_PIECE, plen = min(ADLER_PIECE, I.need - at), o = tid * 16u;
    uint32_t s = 0, t = 0;
    if (o < plen) {
        union { uint4 w; uint8_t b[16]; } v;
        v.w = *reinterpret_cast<const uint4*>(raw + I.raw_begin + at + o);   // (16-byte aligned; the slot has 16 bytes of room behind its end)
        for (uint32_t k = 0; k < 16u; ++k) if (o + k < plen) { s += v.b[k]; t += (plen - (o + k)) * v.b[k]; }
    }
    for (int d = 1; d < (int)WAVE; d <<= 1) { s += __shfl_xor(s, d); t += __shfl_xor(t, d); }   // (t stays below 255 * 4096 * 4097 / 2 < 2^32)
    if ((tid & (WAVE - 1u)) == 0u) { red[2u * (tid / WAVE)] = s; red[2u * (tid / WAVE) + 1u] = t; }
    __syncthreads();
    if (tid == 0u) {
        s = t = 0;
        for (uint32_t w = 0; w < ADLER_THREADS / WAVE; ++w) { s += red[2u * w]; t += red[2u * w + 1u]; }
        parts[g] = make_uint2((1u + s) % ADLER_MOD, (plen + t) % ADLER_MOD);
    }
}
// one wave per file: every lane joins a run of consecutive pieces, then the 64 runs are joined in order
__global__ void __launch_bounds__(WAVE) adler_fold_kernel(const AdlerItem* __restrict__ items, const u64* __restrict__ ptr, const uint2* __restrict__ parts, FileInfo* __restrict__ info) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const AdlerItem I = items[k];
    const uint32_t np = (uint32_t)(ptr[k + 1] - ptr[k]), per = (np + WAVE - 1u) / WAVE;
    uint32_t a = 1, b = 0; u64 len = 0;
    for (uint32_t p = lane * per; p < min(np, (lane + 1u) * per); ++p) {
        const uint2 q = parts[ptr[k] + p];
        const uint32_t plen = min(ADLER_PIECE, I.need - p * ADLER_PIECE);
        adler_join(a, b, q.x, q.y, plen); len += plen;
    }
    uint32_t A = 1, B = 0;
    for (int g = 0; g < (int)WAVE; ++g) adler_join(A, B, __shfl(a, g), __shfl(b, g), (u64)__shfl((uint32_t)len, g));   // (len < 2^31)
    FileInfo& F = info[I.file];
    if (lane == 0u && !F.err && !F.produced_hi && F.produced_lo == I.need && ((B << 16) | A) != F.adler) { F.err = E_ADLER; F.pos = 0; }
}

// ---- unfilter and colour: one wave per file, lane r owns row band + r and works on pixel x = step - r ----
constexpr uint32_t TILE_PITCH = UNFILTER_SEGMENT * 4u + 4u;   // 65 words: the lanes of a step read different banks
__global__ void __launch_bounds__(WAVE) png_unfilter_kernel(const FileDev* __restrict__ files, FileInfo* info, const uint8_t* __restrict__ raw, uint32_t* carry) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[UNFILTER_BAND * TILE_PITCH];
    __shared__ uint32_t above[UNFILTER_SEGMENT];
    __shared__ uint8_t plte[768];
    const FileDev& F = files[blockIdx.x];
    FileInfo& I = info[blockIdx.x];
    if (I.err) return;
    const uint32_t lane = threadIdx.x, W = F.width, H = F.height, bpp = F.bpp, ct = F.colour_type, n_plte = F.n_plte;
    const u64 pitch = 1ull + (u64)W * bpp, row_bytes = (u64)W * bpp;
    const uint8_t* r = raw + F.raw_begin;
    uint32_t* cr = carry + F.carry_begin;
    for (uint32_t k = lane; k < 768u; k += WAVE) plte[k] = F.plte[k];
    uint32_t rows[5] = {0, 0, 0, 0, 0}, bad = 0;
    const uint32_t n_seg = (W + UNFILTER_BAND - 1u + UNFILTER_SEGMENT - 1u) / UNFILTER_SEGMENT;   // steps 0 .. W + 62
    for (uint32_t band = 0; band < H; band += UNFILTER_BAND) {
        const uint32_t y = band + lane;
        const bool live = y < H;
        const uint32_t type = live ? r[(u64)y * pitch] : 0u;
        const u64 refused = __ballot(live && type > 4u);
        if (refused) { if (lane == 0u) { I.err = E_FILTER; I.pos = band + (uint32_t)__builtin_ctzll(refused); } return; }
        for (uint32_t k = 0; k < 5u; ++k) rows[k] += (uint32_t)__popcll(__ballot(live && type == k));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the carried row of the band above is complete
        const bool carries = lane == UNFILTER_BAND - 1u && band + UNFILTER_BAND < H;
        uint8_t* drow = F.dst + (u64)y * W * 3u;
        uint32_t left = 0, upleft = 0, mine = 0;   // a pixel's bytes in one word, byte k = channel k
        for (uint32_t seg = 0; seg < n_seg; ++seg) {
            const uint32_t s0 = seg * UNFILTER_SEGMENT;
            wave_fence();
            for (uint32_t rr = 0; rr < UNFILTER_BAND && band + rr < H; ++rr) {   // row rr's pixels s0 - rr .. s0 - rr + 63
                const uint8_t* in = r + (u64)(band + rr) * pitch + 1u;
                const int64_t first = ((int64_t)s0 - (int64_t)rr) * (int64_t)bpp;
                for (uint32_t j = lane; j < UNFILTER_SEGMENT * bpp; j += WAVE) {
                    const int64_t o = first + j;
                    tile[rr * TILE_PITCH + j] = o >= 0 && (u64)o < row_bytes ? in[o] : (uint8_t)0;
                }
            }
            above[lane] = band && s0 + lane < W ? cr[s0 + lane] : 0u;
            wave_fence();
            for (uint32_t t = 0; t < UNFILTER_SEGMENT; ++t) {
                const uint32_t from_above = __shfl_up(mine, 1);   // the lane above finished this pixel one step ago
                const int64_t x = (int64_t)s0 + t - lane;
                if (!live || x < 0 || x >= (int64_t)W) continue;
                const uint32_t up = lane ? from_above : above[t];
                const uint32_t c = x ? upleft : 0u, a = x ? left : 0u;
                uint32_t cur = 0;
                for (uint32_t k = 0; k < bpp; ++k)
                    cur |= unfilter_byte(type, tile[lane * TILE_PITCH + t * bpp + k], (a >> (8u * k)) & 0xFFu, (up >> (8u * k)) & 0xFFu, (c >> (8u * k)) & 0xFFu) << (8u * k);
                left = cur; upleft = up; mine = cur;
                if (carries) cr[x] = cur;
                uint8_t* o = drow + 3u * (u64)x;
                if (ct == 3u) {
                    const uint32_t e = cur & 0xFFu;
                    if (e >= n_plte) { ++bad; o[0] = o[1] = o[2] = 0; } else { o[0] = plte[3u * e]; o[1] = plte[3u * e + 1u]; o[2] = plte[3u * e + 2u]; }
                } else if (bpp < 3u) o[0] = o[1] = o[2] = (uint8_t)cur;
                else { o[0] = (uint8_t)cur; o[1] = (uint8_t)(cur >> 8); o[2] = (uint8_t)(cur >> 16); }
            }
        }
    }
    u64 bad_all = bad;
    for (int d = 1; d < (int)WAVE; d <<= 1) bad_all += ((u64)__shfl_xor((uint32_t)(bad_all >> 32), d) << 32) + __shfl_xor((uint32_t)bad_all, d);
    if (lane == 0u) {
        for (uint32_t k = 0; k < 5u; ++k) I.rows[k] = rows[k];
        if (bad_all) { I.err = E_PALETTE; I.pos = (uint32_t)min(bad_all, (u64)0xFFFFFFFFu); }
    }
}

}  // namespace

// per-context buffers of the route, allocated on first use
struct PngDecDev { DBuf<uint8_t> z, raw, out; DBuf<uint32_t> carry; DBuf<FileDev> files; DBuf<FileInfo> info; DBuf<uint2> parts; DBuf<AdlerItem> items; DBuf<u64> ptr; };
void pngdec_release(mvs_ctx* ctx) { delete ctx->pngdec; ctx->pngdec = nullptr; }

namespace {

struct HostPng { File F; uint64_t scratch = 0; uint32_t view = 0; };   // view: its number in the caller's list

// the scratch one file needs: its zlib bytes, its inflated stream, a carried row of pixels, 8 bytes per Adler piece, its table entries
uint64_t file_scratch(const File& F) {
    return align16(F.zlib_bytes) + 64u + align16(F.raw_bytes) + 16u + 4ull * F.width + 8ull * ((F.raw_bytes + ADLER_PIECE - 1u) / ADLER_PIECE + 1u) + sizeof(FileDev) + sizeof(FileInfo) + sizeof(AdlerItem) + 8u;
}

// files [a, b) of the call, decoded into dst[a .. b)
void decode_batch(mvs_ctx* ctx, PngDecDev& D, const uint8_t* const* files, const std::vector<HostPng>& H, uint32_t a, uint32_t b, uint8_t* const* dst, const char* who, mvs_pngdec_stats& st) {
    hipStream_t s = ctx->stream;
    const uint32_t n = b - a;
    std::vector<FileDev> fd(n); std::vector<AdlerItem> items(n);
    std::vector<const uint8_t*> src; std::vector<uint8_t*> to; std::vector<size_t> nb;
    uint64_t z_total = 0, raw_total = 0, carry_total = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const File& F = H[a + k].F;
        FileDev& f = fd[k];
        f.z_begin = z_total; f.raw_begin = raw_total; f.z_len = (uint32_t)F.zlib_bytes; f.raw_need = (uint32_t)F.raw_bytes;
        f.width = F.width; f.height = F.height; f.colour_type = F.colour_type; f.bpp = F.bpp; f.n_plte = F.n_plte; f.carry_begin = (uint32_t)carry_total;
        f.dst = dst[a + k];
        memcpy(f.plte, F.plte, 768);
        items[k] = AdlerItem{raw_total, f.raw_need, k};
        z_total += align16(F.zlib_bytes) + 16u; raw_total += align16(F.raw_bytes) + 16u; carry_total += F.width;
        if (carry_total >= 0xFFFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, std::string(who) + ": a batch too large for 32-bit positions (lower max_scratch_bytes)");
        st.idat_chunks += F.idat_chunks; st.zlib_bytes += F.zlib_bytes; st.raw_bytes += F.raw_bytes;
    }
    st.batches += 1;
    D.z.ensure((size_t)z_total + 16); D.raw.ensure((size_t)raw_total + 16); D.carry.ensure((size_t)carry_total + 1); D.info.ensure(n);
    for (uint32_t k = 0; k < n; ++k) {   // the IDAT payloads of a file back to back: its zlib stream
        uint64_t at = fd[k].z_begin;
        for (const Piece& p : H[a + k].F.idat) { src.push_back(files[a + k] + p.off); to.push_back(D.z.p + at); nb.push_back(p.len); at += p.len; }
    }
    StageTimer<5> tm(s);
    tm.mark();
    MVS_HIP(hipMemsetAsync(D.z.p, 0, (size_t)z_total + 16, s));
    MVS_HIP(hipMemsetAsync(D.info.p, 0, n * sizeof(FileInfo), s));
    upload(D.files, fd, s);
    upload_pieces_through_ring(ctx, src.data(), to.data(), nb.data(), src.size());
    MVS_HIP(hipStreamSynchronize(s));
    tm.mark();
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(WAVE), 0, s, (const FileDev*)D.files.p, D.info.p, (const uint8_t*)D.z.p, D.raw.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    auto pieces = [](const AdlerItem& it) { return ((uint64_t)it.need + ADLER_PIECE - 1u) / ADLER_PIECE; };
    uint64_t n_parts = 0;
    for (const AdlerItem& it : items) n_parts += pieces(it);
    D.parts.ensure((size_t)n_parts + 1);
    st.ms_adler += span_launch(s, items, pieces, ADLER_THREADS, ADLER_THREADS, false, D.items, D.ptr, who, [&](unsigned blocks, uint32_t ni, u64) {
        hipLaunchKernelGGL(adler_piece_kernel, dim3(blocks), dim3(ADLER_THREADS), 0, s, (const AdlerItem*)D.items.p, ni, (const u64*)D.ptr.p, (const uint8_t*)D.raw.p, D.parts.p);
    }, [&] {
        hipLaunchKernelGGL(adler_fold_kernel, dim3(n), dim3(WAVE), 0, s, (const AdlerItem*)D.items.p, (const u64*)D.ptr.p, (const uint2*)D.parts.p, D.info.p);
        MVS_LAUNCH_CHECK();
    });
    tm.mark();
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(WAVE), 0, s, (const FileDev*)D.files.p, D.info.p, (const uint8_t*)D.raw.p, D.carry.p);
    MVS_LAUNCH_CHECK();
    tm.mark();
    std::vector<FileInfo> info(n);
    ctx->row_pin.ensure(n * sizeof(FileInfo));
    MVS_HIP(hipMemcpyAsync(ctx->row_pin.p, D.info.p, n * sizeof(FileInfo), hipMemcpyDeviceToHost, s));
    MVS_HIP(hipStreamSynchronize(s));   // (drains the stream: the vectors above were read by asynchronous copies)
    memcpy(info.data(), ctx->row_pin.p, n * sizeof(FileInfo));
    st.ms_upload += tm.ms(0, 1); st.ms_inflate += tm.ms(1, 2); st.ms_unfilter += tm.ms(3, 4);
    for (uint32_t k = 0; k < n; ++k) {
        st.stored_blocks += info[k].blocks[0]; st.fixed_blocks += info[k].blocks[1]; st.dynamic_blocks += info[k].blocks[2];
        for (int t = 0; t < 5; ++t) st.filter_rows[t] += info[k].rows[t];
    }
    for (uint32_t k = 0; k < n; ++k)
        if (info[k].err) {
            const uint64_t at = info[k].err == E_SHORT ? ((uint64_t)info[k].produced_hi << 32 | info[k].produced_lo) : info[k].pos;
            throw StatusError(MVS_ERR_INVALID, std::string(who) + ": view " + std::to_string(H[a + k].view) + ": png: " + refusal(info[k].err, at));
        }
}

// the containers of all files on the host (file k is view view_no[k] of the caller's list; null: view k); with `views`, a frame must have its view's size
std::vector<HostPng> read_containers(const uint8_t* const* files, const uint64_t* sizes, uint32_t n, const uint32_t* view_no, const mvs_view* views, const char* who, mvs_pngdec_stats& st) {
    std::vector<HostPng> H(n);
    for (uint32_t k = 0; k < n; ++k) {
        H[k].view = view_no ? view_no[k] : k;
        const std::string w = std::string(who) + ": view " + std::to_string(H[k].view) + ": ";
        if (!files[k]) throw StatusError(MVS_ERR_INVALID, w + "null file");
        std::string msg;
        if (parse_container(files[k], (size_t)sizes[k], H[k].F, msg) != MVS_OK) throw StatusError(MVS_ERR_INVALID, w + msg);
        const File& F = H[k].F;
        if (views && ((int64_t)F.width != views[H[k].view].width || (int64_t)F.height != views[H[k].view].height))
            throw StatusError(MVS_ERR_INVALID, w + "png: the frame is " + std::to_string(F.width) + " x " + std::to_string(F.height) + ", the view " +
                                                   std::to_string(views[H[k].view].width) + " x " + std::to_string(views[H[k].view].height));
        H[k].scratch = file_scratch(F);
        st.files += 1; st.file_bytes += sizes[k];
    }
    return H;
}
std::vector<size_t> cut_files(const std::vector<HostPng>& H, uint64_t cap, const char* who) {
    std::vector<uint64_t> need(H.size()); std::vector<uint32_t> view(H.size());
    for (size_t k = 0; k < H.size(); ++k) { need[k] = H[k].scratch; view[k] = H[k].view; }
    refuse_over_cap(need, cap, view.data(), who, "scratch");
    return cut_batches(need.data(), need.size(), cap, VIEW_FILES_PER_BATCH);
}
uint64_t scratch_cap(const mvs_jpegdec_params* p) { return p ? p->max_scratch_bytes : VIEW_SCRATCH_DEFAULT; }

}  // namespace

// the PNG views of a scene, some of them through the staging (ctx.h)
void decode_view_pngs(mvs_ctx* ctx, const mvs_view* views, const FileViews& fv, uint8_t* const* dst, const uint8_t* staged, const mvs_jpegdec_params* params, const char* who,
                      mvs_pngdec_stats& st, const StagedBatchFn& after_batch) {
    std::vector<HostPng> H = read_containers(fv.files.data(), fv.sizes.data(), (uint32_t)fv.files.size(), fv.view.data(), views, who, st);
    const size_t n = H.size();
    std::vector<uint64_t> stage_bytes(n);   // a staged file's decoded pixels count towards its scratch
    for (size_t k = 0; k < n; ++k) { stage_bytes[k] = staged[H[k].view] ? 3ull * H[k].F.width * H[k].F.height : 0ull; H[k].scratch += align16(stage_bytes[k]); }
    const std::vector<size_t> cut = cut_files(H, scratch_cap(params), who);
    const BatchLayout L = batch_layout(stage_bytes.data(), n, cut);
    uint8_t* staging = L.most ? view_staging(ctx, L.most) : nullptr;
    std::vector<uint8_t*> to(n);
    for (size_t k = 0; k < n; ++k) to[k] = staged[H[k].view] ? staging + L.off[k] : dst[H[k].view];
    PngDecDev& D = row_dev(ctx->pngdec);
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

mvs_status mvs_ctx_decode_pngs(mvs_ctx* ctx, const uint8_t* const* files, const uint64_t* sizes, uint32_t n, const mvs_jpegdec_params* params, int out_on_device,
                               mvs_rgb_set* out, mvs_pngdec_stats* stats) {
    if (!ctx || !out || (n && (!files || !sizes))) return api_fail(MVS_ERR_INVALID, "null argument");
    *out = mvs_rgb_set{};
    mvs_pngdec_stats st{};
    if (stats) *stats = st;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        run_with_stats(ctx->stream, stats, st, [&] {
            const std::vector<HostPng> H = read_containers(files, sizes, n, nullptr, nullptr, "decode_pngs", st);
            PngDecDev& D = row_dev(ctx->pngdec);
            std::vector<uint32_t> w(n), h(n);
            for (uint32_t k = 0; k < n; ++k) { w[k] = H[k].F.width; h[k] = H[k].F.height; }
            const RgbRoom R = rgb_set_room(D.out, w, h);
            const std::vector<size_t> cut = cut_files(H, scratch_cap(params), "decode_pngs");
            for (size_t k = 0; k + 1 < cut.size(); ++k) decode_batch(ctx, D, files, H, (uint32_t)cut[k], (uint32_t)cut[k + 1], R.dst.data(), "decode_pngs", st);
            rgb_set_out(ctx, D.out, R, w, h, out_on_device, out);
        });
    });
}

mvs_status mvs_scene_set_views_files(mvs_ctx* ctx, const mvs_view* views, uint32_t n_views, const mvs_lens* lens, const uint8_t* const* files, const uint64_t* sizes,
                                     const mvs_jpegdec_params* params, mvs_jpegdec_stats* jpeg_stats, mvs_pngdec_stats* png_stats, mvs_lens_stats* lens_stats) {
    if (!ctx || (n_views && (!views || (files && !sizes)))) return api_fail(MVS_ERR_INVALID, "null argument");
    return set_views_files(ctx, views, n_views, lens, files, sizes, params, jpeg_stats, lens_stats, "set_views_files", "set_views_files", true, png_stats);
}

mvs_status mvs_png_probe(const uint8_t* data, uint64_t size, uint32_t* width, uint32_t* height) {
    if (!data) return api_fail(MVS_ERR_INVALID, "null argument");
    File F; std::string msg;
    if (parse_container(data, (size_t)size, F, msg) != MVS_OK) return api_fail(MVS_ERR_INVALID, msg);
    if (width) *width = F.width;
    if (height) *height = F.height;
    return MVS_OK;
}

mvs_status mvs_decode_png(const uint8_t* data, uint64_t size, uint8_t** rgb, uint32_t* width, uint32_t* height, uint8_t** raw) {
    if (!data || !rgb || !width || !height) return api_fail(MVS_ERR_INVALID, "null argument");
    *rgb = nullptr; *width = *height = 0;
    if (raw) *raw = nullptr;
    std::vector<uint8_t> v, r; std::string msg; uint64_t nb = 0;
    const mvs_status st = decode_png(data, (size_t)size, v, *width, *height, raw ? &r : nullptr, msg);
    if (st == MVS_OK && raw) {
        const mvs_status rr = twin_out(st, msg, r, raw, &nb);
        if (rr != MVS_OK) return rr;
    }
    const mvs_status rc = twin_out(st, msg, v, rgb, &nb);
    if (rc != MVS_OK && raw) { free(*raw); *raw = nullptr; }
    return rc;
}

}  // extern "C"
