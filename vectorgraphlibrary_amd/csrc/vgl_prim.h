// vgl_prim.h -- the device primitives under the builders: scans, sorts, unique, reduce by key and select (rocprim, which no other file of csrc/
// includes), their scratch, the key bits of a sort, the piece plan (vgl_pieces.h), the iota kernel.  Build and plan code only.  DESIGN section 26.
#pragma once
#include "vgl_hip_internal.h"
#include "vgl_pieces.h"
#include <cstring>
#include <iterator>
#include <rocprim/rocprim.hpp>

// The scratch of the primitives: one stream-ordered block that only grows.  0 bytes hold a minimal block too: a null scratch is rocprim's size query.
struct vgl_scratch {
    vgl_dev<char> buf;
    size_t bytes = 0;
    int reserve(hipStream_t st, size_t need) { if (buf.p && need <= bytes) return 0; bytes = need; return buf.alloc(st, need); }
    void reset() { buf.reset(); bytes = 0; }
};
constexpr bool VGL_SIZE_ONLY = true;             // the last argument of a primitive: grow the scratch to what the call needs and run nothing

// call(scratch, bytes) is one rocprim call: asked for its size, given room, and (unless size_only) run.  The timing slot is the caller's.
template <class CALL>
int vgl_prim_call(vgl_hip_ctx *c, vgl_scratch &s, bool size_only, CALL call)
{
    size_t need = 0;
    VGL_HIP_TRY(call((void *)nullptr, need));
    VGL_TRY(s.reserve(c->stream, need));
    if (!size_only) VGL_HIP_TRY(call((void *)s.buf.p, need));
    return 0;
}
template <class IT> using vgl_value_of = typename std::iterator_traits<IT>::value_type;
// input iterators that read no memory: i, and f(i) for a device functor f of an int64_t
template <class T> using vgl_counting = rocprim::counting_iterator<T>;
template <class F> auto vgl_computed(F f) { return rocprim::make_transform_iterator(rocprim::counting_iterator<int64_t>(0), f); }

// Every primitive runs on c->stream over n elements and returns the library's status.  The scans add in the output's type, from 0; in == out is allowed.
template <class IN, class OUT>
int vgl_exclusive_scan(vgl_hip_ctx *c, vgl_scratch &s, IN in, OUT out, size_t n, bool size_only = false)
{
    using T = vgl_value_of<OUT>;
    return vgl_prim_call(c, s, size_only, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, out, (T)0, n, rocprim::plus<T>(), c->stream); });
}
template <class IN, class OUT>
int vgl_inclusive_scan(vgl_hip_ctx *c, vgl_scratch &s, IN in, OUT out, size_t n, bool size_only = false)
{
    using T = vgl_value_of<OUT>;
    return vgl_prim_call(c, s, size_only, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in, out, n, rocprim::plus<T>(), c->stream); });
}
// stable, ascending, over the key bits [begin_bit, end_bit)
template <class KIN, class KOUT, class VIN, class VOUT>
int vgl_sort_pairs(vgl_hip_ctx *c, vgl_scratch &s, KIN keys_in, KOUT keys_out, VIN vals_in, VOUT vals_out, size_t n, unsigned begin_bit, unsigned end_bit, bool size_only = false)
{
    return vgl_prim_call(c, s, size_only, [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, c->stream); });
}
template <class KIN, class KOUT>
int vgl_sort_keys(vgl_hip_ctx *c, vgl_scratch &s, KIN keys_in, KOUT keys_out, size_t n, unsigned begin_bit, unsigned end_bit, bool size_only = false)
{
    return vgl_prim_call(c, s, size_only, [&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, keys_in, keys_out, n, begin_bit, end_bit, c->stream); });
}
// the first element of every run of equal elements; *n_out = their number
template <class IN, class OUT, class COUNT>
int vgl_unique(vgl_hip_ctx *c, vgl_scratch &s, IN in, OUT out, COUNT n_out, size_t n, bool size_only = false)
{
    return vgl_prim_call(c, s, size_only, [&](void *t, size_t &b) { return rocprim::unique(t, b, in, out, n_out, n, rocprim::equal_to<vgl_value_of<IN>>(), c->stream); });
}
// the key and the sum of the values of every run of equal keys; *n_out = the number of runs
template <class KIN, class VIN, class KOUT, class VOUT, class COUNT>
int vgl_reduce_by_key(vgl_hip_ctx *c, vgl_scratch &s, KIN keys_in, VIN vals_in, size_t n, KOUT keys_out, VOUT sums_out, COUNT n_out, bool size_only = false)
{
    return vgl_prim_call(c, s, size_only, [&](void *t, size_t &b) {
        return rocprim::reduce_by_key(t, b, keys_in, vals_in, n, keys_out, sums_out, n_out, rocprim::plus<vgl_value_of<VOUT>>(), rocprim::equal_to<vgl_value_of<KIN>>(), c->stream);
    });
}
// the elements that pred accepts, in their order; *n_out (a size_t) = their number
template <class IN, class OUT, class PRED>
int vgl_select(vgl_hip_ctx *c, vgl_scratch &s, IN in, OUT out, size_t *n_out, size_t n, PRED pred, bool size_only = false)
{
    return vgl_prim_call(c, s, size_only, [&](void *t, size_t &b) { return rocprim::select(t, b, in, out, n_out, n, pred, c->stream); });
}

// The low bits that represent every value up to `largest`: the least b >= 1 with largest < 2^b.  A sort of keys in [0, largest] ends at this bit.
static inline int vgl_key_bits(uint64_t largest)
{
    int bits = 1;
    while (bits < 64 && (largest >> bits) != 0) bits++;
    return bits;
}
// ... that number n values, the keys 0 .. n - 1
static inline int vgl_index_bits(int64_t n) { return vgl_key_bits(n > 1 ? (uint64_t)n - 1 : 0); }

static __global__ __launch_bounds__(VGL_BLOCK) void vgl_k_iota(int32_t n, int32_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) out[i] = (int32_t)i;
}
