// readback.hip -- words from device memory to the host through pinned, coherent memory: a one-block kernel stores them, fences at system
// scope and stores a sequence number the host spins on -- no event in the stream, no drain.  ctx.h says what each entry point is for.
#include "ctx.h"
#include <atomic>

namespace mvs {

namespace {

// one value from device memory into a pinned slot, announced the same way (ICM "moved" counts)
__global__ void report_u32_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t* __restrict__ dst_seq, uint32_t seq) {
    *dst = *src;
    __threadfence_system();
    __hip_atomic_store(dst_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// n <= 64 words from device memory into a pinned buffer, announced like a report (read_words)
__global__ void report_words_kernel(const uint32_t* __restrict__ src, uint32_t n, uint32_t* __restrict__ dst, uint32_t* __restrict__ dst_seq, uint32_t seq) {
    if (threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(dst_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the host's side of an announcement: spins until the pinned word holds the sequence number; `lost` is what to say if the stream went idle without it
void spin_until(mvs_ctx* ctx, const volatile uint32_t* p, uint32_t seq, const char* lost) {
    for (uint64_t spins = 1; *p != seq; ++spins) {
        if ((spins & 0x3FFFu) == 0u) {   // now and then: is the stream still working on it?
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) { if (*p == seq) break; throw HipError(lost); }
            if (q != hipErrorNotReady) MVS_HIP(q);
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
}

}  // namespace

// ---- reports through pinned host memory ----
// Coherent (fine-grained) host memory: a value, a system-scope fence, then the slot's sequence number.  The host spins on the
// number -- no event in the stream (an event record costs the stream ~5 us, and the solver would record one per sweep).
void ensure_report_ring(mvs_ctx* ctx) {
    if (ctx->h_ring) return;
    constexpr uint32_t NS = mvs_ctx::RING + mvs_ctx::ICM_RING;
    MVS_HIP(hipHostMalloc((void**)&ctx->h_ring, (mvs_ctx::RING + 1) * sizeof(mvs_mrf_progress), hipHostMallocCoherent));
    MVS_HIP(hipHostGetDevicePointer((void**)&ctx->d_ring, ctx->h_ring, 0));
    MVS_HIP(hipHostMalloc((void**)&ctx->h_seq, (NS + 2) * sizeof(uint32_t), hipHostMallocCoherent));   // + 2 staging words (mrf_setup)
    MVS_HIP(hipHostGetDevicePointer((void**)&ctx->d_seq, ctx->h_seq, 0));
    MVS_HIP(hipHostMalloc((void**)&ctx->h_icm, mvs_ctx::ICM_RING * sizeof(uint32_t), hipHostMallocCoherent));
    MVS_HIP(hipHostGetDevicePointer((void**)&ctx->d_icm, ctx->h_icm, 0));
    for (uint32_t k = 0; k < NS; ++k) ctx->h_seq[k] = 0u;
    ctx->seq_base = 1u; ctx->icm_seq = 0x40000000u;   // no report carries the initial 0
}
void report_u32(mvs_ctx* ctx, const uint32_t* d_src, uint32_t* d_dst, uint32_t seq_slot, uint32_t seq) {
    hipLaunchKernelGGL(report_u32_kernel, dim3(1), dim3(1), 0, ctx->stream, d_src, d_dst, ctx->d_seq + seq_slot, seq);
    MVS_LAUNCH_CHECK();
}
void read_words(mvs_ctx* ctx, const void* d_src, void* out, uint32_t n_words) {
    if (n_words == 0 || n_words > 64) throw StatusError(MVS_ERR_INVALID, "read_words: 1 .. 64 words");
    if (!ctx->h_rb) {   // 64 data words, the sequence number, and behind it a 4 KB staging area for larger read-backs (read_block)
        MVS_HIP(hipHostMalloc((void**)&ctx->h_rb, (128 + 1024) * sizeof(uint32_t), hipHostMallocCoherent));
        MVS_HIP(hipHostGetDevicePointer((void**)&ctx->d_rb, ctx->h_rb, 0));
        ctx->h_rb[64] = 0u; ctx->rb_seq = 0u;
    }
    const uint32_t seq = ++ctx->rb_seq ? ctx->rb_seq : ++ctx->rb_seq;   // never the initial 0
    hipLaunchKernelGGL(report_words_kernel, dim3(1), dim3(64), 0, ctx->stream, (const uint32_t*)d_src, n_words, ctx->d_rb, ctx->d_rb + 64, seq);
    MVS_LAUNCH_CHECK();
    spin_until(ctx, ctx->h_rb + 64, seq, "a device read-back did not arrive although the stream is idle");
    memcpy(out, ctx->h_rb, n_words * sizeof(uint32_t));
}
// up to 4 KB: through the pinned staging area (a copy into PAGEABLE memory is staged by the driver and costs 10 us more)
void read_block(mvs_ctx* ctx, const void* d_src, void* out, size_t bytes) {
    if (bytes <= 64 * sizeof(uint32_t) && bytes % 4 == 0) { read_words(ctx, d_src, out, (uint32_t)(bytes / 4)); return; }
    if (bytes > 1024 * sizeof(uint32_t)) throw StatusError(MVS_ERR_INVALID, "read_block: at most 4 KB");
    if (!ctx->h_rb) { uint32_t dummy; read_words(ctx, d_src, &dummy, 1); }   // (allocates the pinned area)
    MVS_HIP(hipMemcpyAsync(ctx->h_rb + 128, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, ctx->h_rb + 128, bytes);
}
void wait_report(mvs_ctx* ctx, uint32_t seq_slot, uint32_t seq) {
    spin_until(ctx, ctx->h_seq + seq_slot, seq, "a device report did not arrive although the stream is idle");
}

}  // namespace mvs
