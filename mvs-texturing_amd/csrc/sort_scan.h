// sort_scan.h -- the rocprim two-call idiom, spelled once: size query, the temporary storage grown to it, the run.  Each helper takes the
// temporary buffer and the stream, or a context for its sort_tmp and its stream.  Internal, header-only.
#pragma once
#include "ctx.h"
#include <rocprim/rocprim.hpp>

namespace mvs {

template <class Call>
void with_sort_tmp(DBuf<char>& tmp, Call&& call) {   // call(temporary storage, its size)
    size_t bytes = 0;
    MVS_HIP(call(nullptr, bytes));
    tmp.ensure(bytes + 16);
    MVS_HIP(call(tmp.p, bytes));
}
template <class Call>
void with_sort_tmp(mvs_ctx* ctx, Call&& call) { with_sort_tmp(ctx->sort_tmp, call); }

template <class KeysIn, class KeysOut, class Size>
void dev_sort_keys(DBuf<char>& tmp, hipStream_t s, KeysIn in, KeysOut out, Size n, unsigned begin_bit, unsigned end_bit) {
    with_sort_tmp(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, in, out, n, begin_bit, end_bit, s); });
}
template <class KeysIn, class KeysOut, class Size>
void dev_sort_keys(mvs_ctx* ctx, KeysIn in, KeysOut out, Size n, unsigned begin_bit, unsigned end_bit) {
    dev_sort_keys(ctx->sort_tmp, ctx->stream, in, out, n, begin_bit, end_bit);
}
template <class KeysIn, class KeysOut, class ValsIn, class ValsOut, class Size>
void dev_sort_pairs(DBuf<char>& tmp, hipStream_t s, KeysIn kin, KeysOut kout, ValsIn vin, ValsOut vout, Size n, unsigned begin_bit, unsigned end_bit) {
    with_sort_tmp(tmp, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, n, begin_bit, end_bit, s); });
}
template <class KeysIn, class KeysOut, class ValsIn, class ValsOut, class Size>
void dev_sort_pairs(mvs_ctx* ctx, KeysIn kin, KeysOut kout, ValsIn vin, ValsOut vout, Size n, unsigned begin_bit, unsigned end_bit) {
    dev_sort_pairs(ctx->sort_tmp, ctx->stream, kin, kout, vin, vout, n, begin_bit, end_bit);
}
template <class In, class V>
void dev_exclusive_scan(mvs_ctx* ctx, In in, V* out, size_t n) {   // out[i] = sum of in[0, i) as V
    with_sort_tmp(ctx, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, V(0), n, rocprim::plus<V>(), ctx->stream); });
}

}  // namespace mvs
