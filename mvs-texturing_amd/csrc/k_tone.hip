// k_tone.hip -- tone mapping `gamma` (tone.h; DESIGN.md section 4 "Tone mapping"): the context's texel table that rows f5, f6 and f10 read
//   under the mode, the check of a parameter struct's mode, the route on its own -- gamma_pow on n floats by a plain elementwise kernel
//   (mvs_ctx_gamma_correct) -- and the host twins (mvs_gamma_correct, mvs_tone_table), which compile the same header and need no GPU.
#include "rows.h"
#include "tone.h"
#include <cmath>

namespace mvs {

uint32_t tone_mode(uint32_t tone_mapping, const char* who) {
    if (tone_mapping != TONE_NONE && tone_mapping != TONE_GAMMA)
        throw StatusError(MVS_ERR_INVALID, std::string(who) + ": tone_mapping = " + std::to_string(tone_mapping) + " is neither none (0) nor gamma (1)");
    return tone_mapping;
}

void tone_table_set(mvs_ctx* ctx, const float* table256) {
    float h[256];
    if (table256) memcpy(h, table256, sizeof(h));
    else for (int b = 0; b < 256; ++b) h[b] = tone_table_entry(TONE_GAMMA, b);
    ctx->tone_table.ensure(256);
    MVS_HIP(hipStreamSynchronize(ctx->stream));   // nothing in flight reads the table that is replaced
    MVS_HIP(hipMemcpy(ctx->tone_table.p, h, sizeof(h), hipMemcpyHostToDevice));
    ctx->tone_table_valid = true;
}

const float* tone_table_dev(mvs_ctx* ctx) {
    if (!ctx->tone_table_valid) tone_table_set(ctx, nullptr);   // the table is data: built on the host, uploaded once per context
    return ctx->tone_table.p;
}

namespace {
// four values per thread where the array allows 16-byte accesses, the rest one by one
__global__ void __launch_bounds__(256) gamma_correct_kernel(float* __restrict__ v, unsigned long long n, unsigned long long nvec, float power) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t < nvec) {
        float4 q = reinterpret_cast<float4*>(v)[t];
        q.x = gamma_pow(q.x, power); q.y = gamma_pow(q.y, power); q.z = gamma_pow(q.z, power); q.w = gamma_pow(q.w, power);
        reinterpret_cast<float4*>(v)[t] = q;
        return;
    }
    const unsigned long long i = 4ull * nvec + (t - nvec);
    if (i < n) v[i] = gamma_pow(v[i], power);
}
bool power_ok(float power) { return std::isfinite(power) && power > 0.0f; }
}  // namespace
}  // namespace mvs

using namespace mvs;

extern "C" {

mvs_status mvs_gamma_correct(float* values, uint64_t n, float power) {
    if (n && !values) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!power_ok(power)) return api_fail(MVS_ERR_INVALID, "gamma_correct: the power must be finite and > 0");
    for (uint64_t i = 0; i < n; ++i) values[i] = gamma_pow(values[i], power);
    return MVS_OK;
}

mvs_status mvs_tone_table(uint32_t mode, float out[256]) {
    if (!out) return api_fail(MVS_ERR_INVALID, "null argument");
    if (mode != TONE_NONE && mode != TONE_GAMMA) return api_fail(MVS_ERR_INVALID, "tone_table: the mode is neither none (0) nor gamma (1)");
    for (int b = 0; b < 256; ++b) out[b] = tone_table_entry((int)mode, b);
    return MVS_OK;
}

mvs_status mvs_ctx_gamma_correct(mvs_ctx* ctx, float* values, uint64_t n, float power, int on_device) {
    if (!ctx || (n && !values)) return api_fail(MVS_ERR_INVALID, "null argument");
    if (!power_ok(power)) return api_fail(MVS_ERR_INVALID, "gamma_correct: the power must be finite and > 0");
    if (!n) return MVS_OK;
    return api_guard([&] {
        MVS_HIP(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        DBuf<float> tmp;
        float* d = values;
        if (!on_device) {
            tmp.ensure((size_t)n);
            d = tmp.p;
            MVS_HIP(hipMemcpyAsync(d, values, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        }
        const unsigned long long nvec = ((uintptr_t)d & 15u) ? 0ull : n / 4ull, threads = nvec + (n - 4ull * nvec);
        if ((threads + 255ull) / 256ull >= 0x7FFFFFFFull) throw StatusError(MVS_ERR_UNSUPPORTED, "gamma_correct: too many values for one call");
        {
            Prof pr(ctx, "gamma_correct");   // option "profile": the kernel's device time (mvs_ctx_get_profile)
            hipLaunchKernelGGL(gamma_correct_kernel, dim3(grid((size_t)threads)), dim3(256), 0, s, d, (unsigned long long)n, nvec, power);
            MVS_LAUNCH_CHECK();
        }
        if (!on_device) MVS_HIP(hipMemcpyAsync(values, d, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        MVS_HIP(hipStreamSynchronize(s));   // the caller's host buffer is borrowed for the call only; tmp is freed on return
    });
}

}  // extern "C"
