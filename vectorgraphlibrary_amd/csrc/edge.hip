// edge.hip -- one float32 per stored entry of an aggregation plan (agg.hip): the dot product of a feature row of the entry's row with a feature row of
// its column (SDDMM), the softmax of such scalars over each row, and the backward of that softmax.  With the two runs of agg.hip they close the
// gradients of a weighted aggregation: the gradient with respect to the weights IS the dot product of (grad_out, x), the gradients of the dot product
// ARE the forward and the transposed run with the incoming entry gradient as the weight.  The contract is written out in include/vgl_hip.h; DESIGN
// section 30 has the kernels, their resources, the bytes model, the tolerances and the measurements.
//
//   dot      the team kernel of the aggregation turned round: the lanes of a team are (entry slot x column group), NQ lanes cover a tile of NQ * VEC
//            columns, slot s takes entries s, s + SLOTS, ... with four gathers of b in flight; a lane adds its VEC products in column order, tile
//            after tile, and the NQ lanes of an entry are folded by an xor butterfly at offsets 1, 2, ... NQ / 2; lane q = 0 stores e[p].  The row's
//            own a stays in registers with one column tile and is re-read per tile (from cache) with more.  Chunks only divide the work.
//   rows     softmax and its backward: every lane an entry slot.  A row of one chunk is finished by its team (walks: max, sum, write; backward: sum,
//            write).  A chunk of a longer row leaves (m_c, s_c) (backward: d_c); vgl_k_edge_hubs, a thread per such row, merges them in chunk order
//            and leaves the row's (M, S) in every one of its chunks' slots; vgl_k_edge_hub_write writes the entries, a workgroup per chunk.
//   heads    the same three calls on H scalars per entry, e[p * H + h], head h on the columns [h D, (h + 1) D): separate kernels
//            (vgl_k_edge_dot_heads, vgl_k_edge_rows_heads, ...) further down, so that the single-head instantiations stay as they were; each head
//            has the bits of the single-head call on its column slice.
//   gat      the additive score e[p, h] = leaky_relu(s[row(p), h] + t[adj[p], h]) on the same E x H layout, and the sums of (gated) entry scalars
//            over the rows or, through the transpose, over the columns, which are its gradients: vgl_k_edge_add_heads,
//            vgl_k_edge_sum_heads, vgl_k_edge_sum_hubs at the end of the kernels.
// Every value has one writer and every sum a shape fixed by (row length, F, VEC, the three switches): no floating-point atomic, no scratch memory, no
// cooperative launch, no wait on a flag, no retry loop.
#include "vgl_agg.h"
#include <cmath>
#include <cstring>
#include <string>

namespace {

struct edge_dot_args {
    const int64_t *rowptr;
    const int32_t *adj;
    const float *a, *b;          // n_rows x F (lda), n_cols x F (ldb)
    float *e;                    // one per entry
    int64_t lda, ldb;
    int32_t F, chunk;
    int32_t lognq[VGL_RC_N], tiles[VGL_RC_N];
    int32_t mean;                // divide the finished dot by the row's length
};

template <int CLS, int VEC>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_dot(agg_list l, int32_t n, edge_dot_args a)
{
    using T = vgl_rc_team<CLS>;
    const int lognq = a.lognq[CLS], nq = 1 << lognq, slots = T::LANES >> lognq;
    const int q = T::lane() & (nq - 1), slot = T::lane() >> lognq;
    const bool one = a.tiles[CLS] == 1;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int32_t v = 0;
        int64_t lo = 0, hi = 0, len = 0;
        if (has) {
            v = l.rows[i];
            lo = a.rowptr[v]; hi = a.rowptr[v + 1];
            len = hi - lo;
            if constexpr (CLS == VGL_RC_WG) {
                const int64_t end = hi;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        const float *arow = a.a + (int64_t)v * a.lda;
        float av[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) av[k] = 0.0f;
        if (one && q * VEC < a.F && lo < hi) agg_load<VEC>(arow + q * VEC, av);     // one tile: the row's values stay in registers
        int64_t p = lo + slot;
        // the NQ lanes of a slot share p: they stay together through the loops and the butterfly, a lane past the last column loads nothing
        for (; p + 3 * (int64_t)slots < hi; p += 4 * (int64_t)slots) {                 // four gathers in flight
            int32_t u[4];
            float acc[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { u[j] = a.adj[p + j * (int64_t)slots]; acc[j] = 0.0f; }
            for (int base = 0; base < a.F; base += nq * VEC) {
                const int c0 = base + q * VEC;
                if (c0 < a.F) {
                    float t[4][VEC];
#pragma unroll
                    for (int j = 0; j < 4; j++) agg_load<VEC>(a.b + (int64_t)u[j] * a.ldb + c0, t[j]);
                    if (!one) agg_load<VEC>(arow + c0, av);
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int k = 0; k < VEC; k++) acc[j] = acc[j] + av[k] * t[j][k];
                }
            }
            for (int o = 1; o < nq; o <<= 1)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[j] = acc[j] + __shfl_xor(acc[j], o);
            if (q == 0)
#pragma unroll
                for (int j = 0; j < 4; j++) a.e[p + j * (int64_t)slots] = a.mean ? acc[j] / (float)len : acc[j];
        }
        for (; p < hi; p += slots) {
            const int32_t u = a.adj[p];
            float acc = 0.0f;
            for (int base = 0; base < a.F; base += nq * VEC) {
                const int c0 = base + q * VEC;
                if (c0 < a.F) {
                    float t[VEC];
                    agg_load<VEC>(a.b + (int64_t)u * a.ldb + c0, t);
                    if (!one) agg_load<VEC>(arow + c0, av);
#pragma unroll
                    for (int k = 0; k < VEC; k++) acc = acc + av[k] * t[k];
                }
            }
            for (int o = 1; o < nq; o <<= 1) acc = acc + __shfl_xor(acc, o);
            if (q == 0) a.e[p] = a.mean ? acc / (float)len : acc;
        }
    }
}

// ---- softmax over the rows and its backward ----
struct edge_rows_args {
    const int64_t *rowptr;
    const float *x, *g;          // forward: x = e; backward: x = y, g = gy
    float *out;                  // y; backward: ge
    float2 *part;                // per workgroup item, for the rows of more than one chunk: (m_c, s_c); backward (d_c, 0); then the row's (M, S) / (d, 0)
    int32_t chunk;
};

// the sum of v over the team, in every lane: an xor butterfly at offsets 1, 2, ... inside the wave, then the workgroup's waves in wave order
template <int CLS>
__device__ __forceinline__ float edge_team_sum(float v)
{
    constexpr int FOLD = vgl_rc_team<CLS>::LANES < 64 ? vgl_rc_team<CLS>::LANES : 64;
#pragma unroll
    for (int o = 1; o < FOLD; o <<= 1) v = v + __shfl_xor(v, o);
    if constexpr (CLS == VGL_RC_WG) {
        __shared__ float s_sum[VGL_WAVES];
        __syncthreads();                                              // the sums of the item before have been read
        if (vgl_lane() == 0) s_sum[vgl_wave()] = v;
        __syncthreads();
        v = s_sum[0];
#pragma unroll
        for (int w = 1; w < VGL_WAVES; w++) v = v + s_sum[w];
    }
    return v;
}

// the entries first, first + step, ... below hi, given the row's (m, s) (backward: d in s)
template <bool BWD>
__device__ __forceinline__ void edge_write(const edge_rows_args &a, int64_t first, int64_t hi, int step, float m, float s)
{
    if constexpr (BWD) {
        for (int64_t p = first; p < hi; p += step) a.out[p] = a.x[p] * (a.g[p] - s);
    } else {
        const bool dead = m == -INFINITY;                             // every entry of the row is at -inf
        for (int64_t p = first; p < hi; p += step) a.out[p] = dead ? 0.0f : expf(a.x[p] - m) / s;
    }
}

template <int CLS, bool BWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_rows(agg_list l, int32_t n, edge_rows_args a)
{
    using T = vgl_rc_team<CLS>;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int64_t lo = 0, hi = 0;
        bool whole = true;
        if (has) {
            const int32_t v = l.rows[i];
            lo = a.rowptr[v]; hi = a.rowptr[v + 1];
            if constexpr (CLS == VGL_RC_WG) {
                const int64_t end = hi;
                whole = hi - lo <= a.chunk;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        const int64_t first = lo + T::lane();
        float m = 0.0f, acc = 0.0f;
        if constexpr (BWD) {
            for (int64_t p = first; p < hi; p += T::LANES) acc = acc + a.x[p] * a.g[p];
        } else {
            float mx = -INFINITY;
            for (int64_t p = first; p < hi; p += T::LANES) { const float x = a.x[p]; mx = x > mx ? x : mx; }
            m = T::max_of(mx);
            if (m != -INFINITY)                                       // (else every term is 0, and -inf - -inf is not formed)
                for (int64_t p = first; p < hi; p += T::LANES) acc = acc + expf(a.x[p] - m);
        }
        const float s = edge_team_sum<CLS>(acc);
        if (CLS == VGL_RC_WG && !whole) {
            if (T::lead() && has) a.part[i] = make_float2(BWD ? s : m, BWD ? 0.0f : s);
        } else edge_write<BWD>(a, first, hi, T::LANES, m, s);
    }
}

// the rows of more than one chunk: a thread per row merges its chunks' partials in chunk order and leaves the row's pair in each of their slots
struct edge_hubs { const int32_t *first, *nch; int32_t n; };
template <bool BWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_hubs(edge_hubs h, float2 *part)
{
    for (int64_t k = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; k < h.n; k += (int64_t)gridDim.x * VGL_BLOCK) {
        float2 *mine = part + h.first[k];
        const int32_t nch = h.nch[k];
        float m = 0.0f, s = 0.0f;
        if constexpr (BWD) {
            s = mine[0].x;
            for (int32_t j = 1; j < nch; j++) s = s + mine[j].x;
        } else {
            m = mine[0].x;
            for (int32_t j = 1; j < nch; j++) m = mine[j].x > m ? mine[j].x : m;
            for (int32_t j = 0; j < nch; j++) {
                const float2 c = mine[j];
                if (c.x != -INFINITY) s = s + c.y * expf(c.x - m);    // a chunk of -inf alone contributes nothing
            }
        }
        for (int32_t j = 0; j < nch; j++) mine[j] = make_float2(BWD ? s : m, BWD ? 0.0f : s);
    }
}
// ... and a workgroup per chunk of such a row writes its entries (the items of rows of one chunk were finished by vgl_k_edge_rows)
template <bool BWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_hub_write(agg_list l, int32_t n, edge_rows_args a)
{
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t v = l.rows[i];
        const int64_t row_lo = a.rowptr[v], end = a.rowptr[v + 1];
        if (end - row_lo <= a.chunk) continue;                        // (uniform over the workgroup)
        const int64_t lo = row_lo + (int64_t)l.chunk[i] * a.chunk, hi = min(end, lo + a.chunk);
        const float2 ms = a.part[i];
        edge_write<BWD>(a, lo + threadIdx.x, hi, VGL_BLOCK, ms.x, BWD ? ms.x : ms.y);      // (M, S); backward: d in the first
    }
}

// ---- heads: H scalars per entry, e[p * H + h]; head h owns the columns [h D, (h + 1) D) ----
// The dot product: the lanes of an entry slot are (head of the pass x column group of the head).  NQ lanes per head and the tiles of a head come from
// agg_shape(D, VEC), HP heads sit beside each other (a power of two: what the class's lane budget holds, no more than H needs), the remaining heads
// follow in further passes over the same adj[p].  The butterfly stops at NQ / 2, so it folds the lanes of one head only and e[:, h] has the bits of
// vgl_k_edge_dot at width D on the head's column slice.
struct edge_dot_heads_args {
    const int64_t *rowptr;
    const int32_t *adj;
    const float *a, *b;          // n_rows x F (lda), n_cols x F (ldb), F = H * D
    float *e;                    // E x H
    int64_t lda, ldb;
    int32_t H, D, chunk;
    int32_t lognq[VGL_RC_N], tiles[VGL_RC_N];    // of one head: agg_shape(D, VEC)
    int32_t loghp[VGL_RC_N], passes[VGL_RC_N];   // heads beside each other in a slot, passes over the heads
    int32_t mean;
};

template <int CLS, int VEC>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_dot_heads(agg_list l, int32_t n, edge_dot_heads_args a)
{
    using T = vgl_rc_team<CLS>;
    const int lognq = a.lognq[CLS], nq = 1 << lognq, hp = 1 << a.loghp[CLS], logw = lognq + a.loghp[CLS], slots = T::LANES >> logw;
    const int q = T::lane() & (nq - 1), hl = (T::lane() >> lognq) & (hp - 1), slot = T::lane() >> logw;
    const int tiles = a.tiles[CLS], passes = a.passes[CLS], cq = q * VEC;
    const bool one = tiles == 1 && passes == 1;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int32_t v = 0;
        int64_t lo = 0, hi = 0, len = 0;
        if (has) {
            v = l.rows[i];
            lo = a.rowptr[v]; hi = a.rowptr[v + 1];
            len = hi - lo;
            if constexpr (CLS == VGL_RC_WG) {
                const int64_t end = hi;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        const float *arow = a.a + (int64_t)v * a.lda;
        float av[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) av[k] = 0.0f;
        if (one && hl < a.H && cq < a.D && lo < hi) agg_load<VEC>(arow + hl * a.D + cq, av);      // one pass of one tile: the row's values stay in registers
        int64_t p = lo + slot;
        // the lanes of a slot share p: they stay together through the loops and the butterflies; a lane past the last head or column loads nothing
        for (; p + 3 * (int64_t)slots < hi; p += 4 * (int64_t)slots) {                 // four gathers in flight, adj read once for every pass
            int32_t u[4];
#pragma unroll
            for (int j = 0; j < 4; j++) u[j] = a.adj[p + j * (int64_t)slots];
            for (int ps = 0; ps < passes; ps++) {
                const int h = ps * hp + hl;
                const bool hact = h < a.H;
                float acc[4];
#pragma unroll
                for (int j = 0; j < 4; j++) acc[j] = 0.0f;
                for (int t = 0, c = cq; t < tiles; t++, c += nq * VEC) {
                    if (hact && c < a.D) {
                        const int c0 = h * a.D + c;
                        float x[4][VEC];
#pragma unroll
                        for (int j = 0; j < 4; j++) agg_load<VEC>(a.b + (int64_t)u[j] * a.ldb + c0, x[j]);
                        if (!one) agg_load<VEC>(arow + c0, av);
#pragma unroll
                        for (int j = 0; j < 4; j++)
#pragma unroll
                            for (int k = 0; k < VEC; k++) acc[j] = acc[j] + av[k] * x[j][k];
                    }
                }
                for (int o = 1; o < nq; o <<= 1)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[j] = acc[j] + __shfl_xor(acc[j], o);
                if (q == 0 && hact)
#pragma unroll
                    for (int j = 0; j < 4; j++) a.e[(p + j * (int64_t)slots) * a.H + h] = a.mean ? acc[j] / (float)len : acc[j];
            }
        }
        for (; p < hi; p += slots) {
            const int32_t u = a.adj[p];
            for (int ps = 0; ps < passes; ps++) {
                const int h = ps * hp + hl;
                const bool hact = h < a.H;
                float acc = 0.0f;
                for (int t = 0, c = cq; t < tiles; t++, c += nq * VEC) {
                    if (hact && c < a.D) {
                        const int c0 = h * a.D + c;
                        float x[VEC];
                        agg_load<VEC>(a.b + (int64_t)u * a.ldb + c0, x);
                        if (!one) agg_load<VEC>(arow + c0, av);
#pragma unroll
                        for (int k = 0; k < VEC; k++) acc = acc + av[k] * x[k];
                    }
                }
                for (int o = 1; o < nq; o <<= 1) acc = acc + __shfl_xor(acc, o);
                if (q == 0 && hact) a.e[p * a.H + h] = a.mean ? acc / (float)len : acc;
            }
        }
    }
}

// The softmax and its backward: every lane an entry slot that carries a block of HB heads in registers; HB divides H, the blocks follow each other.
struct edge_rows_heads_args {
    const int64_t *rowptr;
    const float *x, *g;          // E x H.  forward: x = e; backward: x = y, g = gy
    float *out;                  // E x H: y; backward: ge
    float2 *part;                // per (workgroup item, head), as in edge_rows_args
    int32_t chunk, H;
    int32_t wide;                // x, g and out are 16-byte aligned: a lane's block of heads goes as 8- or 16-byte accesses
};

template <int HB> __device__ __forceinline__ void edge_load_heads(const float *p, bool wide, float *v)
{
    if constexpr (HB >= 4) {
        if (wide) {
#pragma unroll
            for (int k = 0; k < HB; k += 4) agg_load<4>(p + k, v + k);
            return;
        }
    } else if constexpr (HB == 2) {
        if (wide) { const float2 t = *reinterpret_cast<const float2 *>(p); v[0] = t.x; v[1] = t.y; return; }
    }
#pragma unroll
    for (int k = 0; k < HB; k++) v[k] = p[k];
}
template <int HB> __device__ __forceinline__ void edge_store_heads(float *p, bool wide, const float *v)
{
    if constexpr (HB >= 4) {
        if (wide) {
#pragma unroll
            for (int k = 0; k < HB; k += 4) agg_store<4>(p + k, v + k);
            return;
        }
    } else if constexpr (HB == 2) {
        if (wide) { *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]); return; }
    }
#pragma unroll
    for (int k = 0; k < HB; k++) p[k] = v[k];
}

// edge_team_sum for HB values at once: the same butterfly and the same wave order per value, one pair of barriers for the block
template <int CLS, int HB>
__device__ __forceinline__ void edge_team_sum_heads(float *v)
{
    constexpr int FOLD = vgl_rc_team<CLS>::LANES < 64 ? vgl_rc_team<CLS>::LANES : 64;
#pragma unroll
    for (int k = 0; k < HB; k++)
#pragma unroll
        for (int o = 1; o < FOLD; o <<= 1) v[k] = v[k] + __shfl_xor(v[k], o);
    if constexpr (CLS == VGL_RC_WG) {
        __shared__ float s_sum[VGL_WAVES][HB];
        __syncthreads();                                              // the sums of the block before have been read
        if (vgl_lane() == 0)
#pragma unroll
            for (int k = 0; k < HB; k++) s_sum[vgl_wave()][k] = v[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < HB; k++) {
            v[k] = s_sum[0][k];
#pragma unroll
            for (int w = 1; w < VGL_WAVES; w++) v[k] = v[k] + s_sum[w][k];
        }
    }
}
// the largest of each of HB values over the team, in every lane (a maximum has no rounding: its shape is free)
template <int CLS, int HB>
__device__ __forceinline__ void edge_team_max_heads(float *v)
{
    constexpr int FOLD = vgl_rc_team<CLS>::LANES < 64 ? vgl_rc_team<CLS>::LANES : 64;
#pragma unroll
    for (int k = 0; k < HB; k++)
#pragma unroll
        for (int o = 1; o < FOLD; o <<= 1) { const float t = __shfl_xor(v[k], o); v[k] = t > v[k] ? t : v[k]; }
    if constexpr (CLS == VGL_RC_WG) {
        __shared__ float s_max[VGL_WAVES][HB];
        __syncthreads();                                              // the maxima of the block before have been read
        if (vgl_lane() == 0)
#pragma unroll
            for (int k = 0; k < HB; k++) s_max[vgl_wave()][k] = v[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < HB; k++)
#pragma unroll
            for (int w = 0; w < VGL_WAVES; w++) v[k] = s_max[w][k] > v[k] ? s_max[w][k] : v[k];
    }
}

// the heads h0 .. h0 + HB - 1 of the entries first, first + step, ... below hi, given (m, s) per head (backward: d in s)
template <bool BWD, int HB>
__device__ __forceinline__ void edge_write_heads(const edge_rows_heads_args &a, int64_t first, int64_t hi, int step, int h0, const float *m, const float *s)
{
    const bool wide = a.wide != 0;
    for (int64_t p = first; p < hi; p += step) {
        const int64_t at = p * a.H + h0;
        float x[HB], r[HB];
        edge_load_heads<HB>(a.x + at, wide, x);
        if constexpr (BWD) {
            float g[HB];
            edge_load_heads<HB>(a.g + at, wide, g);
#pragma unroll
            for (int k = 0; k < HB; k++) r[k] = x[k] * (g[k] - s[k]);
        } else {
#pragma unroll
            for (int k = 0; k < HB; k++) r[k] = m[k] == -INFINITY ? 0.0f : expf(x[k] - m[k]) / s[k];      // (a head whose row is at -inf alone: 0)
        }
        edge_store_heads<HB>(a.out + at, wide, r);
    }
}

template <int CLS, bool BWD, int HB>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_rows_heads(agg_list l, int32_t n, edge_rows_heads_args a)
{
    using T = vgl_rc_team<CLS>;
    const bool wide = a.wide != 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int64_t lo = 0, hi = 0;
        bool whole = true;
        if (has) {
            const int32_t v = l.rows[i];
            lo = a.rowptr[v]; hi = a.rowptr[v + 1];
            if constexpr (CLS == VGL_RC_WG) {
                const int64_t end = hi;
                whole = hi - lo <= a.chunk;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        const int64_t first = lo + T::lane();
        for (int h0 = 0; h0 < a.H; h0 += HB) {                         // the blocks of heads: the same trips in every lane
            float m[HB], acc[HB];
#pragma unroll
            for (int k = 0; k < HB; k++) { m[k] = 0.0f; acc[k] = 0.0f; }
            if constexpr (BWD) {
                for (int64_t p = first; p < hi; p += T::LANES) {
                    float x[HB], g[HB];
                    edge_load_heads<HB>(a.x + p * a.H + h0, wide, x);
                    edge_load_heads<HB>(a.g + p * a.H + h0, wide, g);
#pragma unroll
                    for (int k = 0; k < HB; k++) acc[k] = acc[k] + x[k] * g[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < HB; k++) m[k] = -INFINITY;
                for (int64_t p = first; p < hi; p += T::LANES) {
                    float x[HB];
                    edge_load_heads<HB>(a.x + p * a.H + h0, wide, x);
#pragma unroll
                    for (int k = 0; k < HB; k++) m[k] = x[k] > m[k] ? x[k] : m[k];
                }
                edge_team_max_heads<CLS, HB>(m);
                for (int64_t p = first; p < hi; p += T::LANES) {
                    float x[HB];
                    edge_load_heads<HB>(a.x + p * a.H + h0, wide, x);
#pragma unroll
                    for (int k = 0; k < HB; k++)
                        if (m[k] != -INFINITY) acc[k] = acc[k] + expf(x[k] - m[k]);      // (else every term is 0, and -inf - -inf is not formed)
                }
            }
            edge_team_sum_heads<CLS, HB>(acc);
            if (CLS == VGL_RC_WG && !whole) {
                if (T::lead() && has)
#pragma unroll
                    for (int k = 0; k < HB; k++) a.part[i * a.H + h0 + k] = make_float2(BWD ? acc[k] : m[k], BWD ? 0.0f : acc[k]);
            } else edge_write_heads<BWD, HB>(a, first, hi, T::LANES, h0, m, acc);
        }
    }
}

// the rows of more than one chunk: a thread per (row, head) merges the head's partials in chunk order, as vgl_k_edge_hubs does for one head
template <bool BWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_hubs_heads(edge_hubs h, int32_t H, float2 *part)
{
    const int64_t total = (int64_t)h.n * H;
    for (int64_t t = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t k = (int32_t)(t / H);
        float2 *mine = part + (int64_t)h.first[k] * H + (t - (int64_t)k * H);
        const int32_t nch = h.nch[k];
        float m = 0.0f, s = 0.0f;
        if constexpr (BWD) {
            s = mine[0].x;
            for (int32_t j = 1; j < nch; j++) s = s + mine[(int64_t)j * H].x;
        } else {
            m = mine[0].x;
            for (int32_t j = 1; j < nch; j++) m = mine[(int64_t)j * H].x > m ? mine[(int64_t)j * H].x : m;
            for (int32_t j = 0; j < nch; j++) {
                const float2 c = mine[(int64_t)j * H];
                if (c.x != -INFINITY) s = s + c.y * expf(c.x - m);    // a chunk of -inf alone contributes nothing
            }
        }
        for (int32_t j = 0; j < nch; j++) mine[(int64_t)j * H] = make_float2(BWD ? s : m, BWD ? 0.0f : s);
    }
}
template <bool BWD, int HB>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_hub_write_heads(agg_list l, int32_t n, edge_rows_heads_args a)
{
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t v = l.rows[i];
        const int64_t row_lo = a.rowptr[v], end = a.rowptr[v + 1];
        if (end - row_lo <= a.chunk) continue;                        // (uniform over the workgroup)
        const int64_t lo = row_lo + (int64_t)l.chunk[i] * a.chunk, hi = min(end, lo + a.chunk);
        for (int h0 = 0; h0 < a.H; h0 += HB) {
            float m[HB], s[HB];
#pragma unroll
            for (int k = 0; k < HB; k++) { const float2 ms = a.part[i * a.H + h0 + k]; m[k] = ms.x; s[k] = BWD ? ms.x : ms.y; }
            edge_write_heads<BWD, HB>(a, lo + threadIdx.x, hi, VGL_BLOCK, h0, m, s);
        }
    }
}

// the stats of a run over the plan's CSR; `per_entry` bytes per entry beside the adjacency walks, `per_row` per row beside the list entries
void edge_stats(const vgl_hip_agg_plan *p, const int32_t *tiles, int vec, int64_t adj_bytes, int64_t per_entry, int64_t per_row, vgl_hip_agg_stats *stats, int32_t heads = 0)
{
    const vgl_agg_lists &L = p->fwd;
    vgl_hip_agg_stats s;
    memset(&s, 0, sizeof(s));
    s.rows = p->n_rows; s.entries = L.entries;
    s.rows_short = L.rows_of[0]; s.rows_wave = L.rows_of[1]; s.rows_wg = L.rows_of[2];
    s.chunks = L.n[VGL_RC_WG]; s.hub_rows = L.nhubs;
    s.transposed = 0; s.vec = vec; s.heads = heads;
    int64_t bytes = 0;
    for (int q = 0; q < VGL_RC_N; q++) { s.column_tiles[q] = tiles[q]; bytes += L.entries_of[q] * tiles[q] * adj_bytes; }
    bytes += L.entries * per_entry + (int64_t)p->n_rows * per_row;
    bytes += 4 * (L.rows_of[0] + L.rows_of[1]) + 8 * L.n[VGL_RC_WG];
    s.algorithmic_bytes = bytes;
    *stats = s;
}

int edge_check_call(const char *who, vgl_hip_ctx *c, vgl_hip_agg_plan *p, const void *x, const void *y, const void *z)
{
    static thread_local std::string msg;
    auto fail = [&](const char *what) { msg = std::string(who) + ": " + what; return vgl_set_error(__FILE__, __LINE__, msg.c_str()); };
    if (!c || !p || !x || !y || !z) return fail("null argument");
    if (p->c != c) return fail("the plan belongs to another context");
    return 0;
}

template <bool BWD>
int edge_rows_run(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_x, const float *d_g, float *d_out, vgl_hip_agg_stats *stats)
{
    VGL_HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const vgl_agg_lists &L = p->fwd;
    edge_rows_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->rowptr; a.x = d_x; a.g = d_g; a.out = d_out;
    a.chunk = L.ch.chunk;
    vgl_dev<float> part;
    if (L.nhubs > 0) VGL_TRY(part.alloc(st, 2 * (size_t)L.n[VGL_RC_WG]));
    a.part = reinterpret_cast<float2 *>(part.p);
    const char *const slot[VGL_RC_N] = {"edge_short", "edge_wave", "edge_wg"};
    const agg_list list[VGL_RC_N] = {{L.rows.p, nullptr}, {L.rows.p + L.n[0], nullptr}, {L.item_row.p, L.item_chunk.p}};
    VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_rows<VGL_RC_SHORT, BWD>, vgl_k_edge_rows<VGL_RC_WAVE, BWD>, vgl_k_edge_rows<VGL_RC_WG, BWD>, list, a));
    if (L.nhubs > 0) {
        const edge_hubs hubs{L.hub_first.p, L.hub_nch.p, (int32_t)L.nhubs};
        {
            vgl_timed_launch tl(c, "edge_hubs");
            hipLaunchKernelGGL(vgl_k_edge_hubs<BWD>, dim3(vgl_grid(L.nhubs, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, hubs, a.part);
        }
        vgl_timed_launch tl(c, "edge_hub_write");
        hipLaunchKernelGGL(vgl_k_edge_hub_write<BWD>, dim3(vgl_grid(L.n[VGL_RC_WG], 1, agg_grid_cap[VGL_RC_WG])), dim3(VGL_BLOCK), 0, st, list[VGL_RC_WG], (int32_t)L.n[VGL_RC_WG], a);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // (the partials are free again; the result is there when the call returns)
    if (stats) {
        const int32_t tiles[VGL_RC_N] = {1, 1, 1};
        // forward: three walks of e and y written; backward: two walks of y and gy and ge written; 8 bytes of bounds per row
        edge_stats(p, tiles, 1, 0, BWD ? 8 * 2 + 4 : 4 * 3 + 4, 8, stats);
    }
    return 0;
}

// the largest of 8, 4, 2, 1 that divides H: the heads a lane carries at a time
int edge_head_block(int32_t H) { return H % 8 == 0 ? 8 : H % 4 == 0 ? 4 : H % 2 == 0 ? 2 : 1; }

template <bool BWD, int HB>
int edge_rows_heads_launch(vgl_hip_ctx *c, const vgl_agg_lists &L, const edge_rows_heads_args &a)
{
    hipStream_t st = c->stream;
    const char *const slot[VGL_RC_N] = {"edge_short", "edge_wave", "edge_wg"};
    const agg_list list[VGL_RC_N] = {{L.rows.p, nullptr}, {L.rows.p + L.n[0], nullptr}, {L.item_row.p, L.item_chunk.p}};
    VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_rows_heads<VGL_RC_SHORT, BWD, HB>, vgl_k_edge_rows_heads<VGL_RC_WAVE, BWD, HB>,
                               vgl_k_edge_rows_heads<VGL_RC_WG, BWD, HB>, list, a));
    if (L.nhubs > 0) {
        const edge_hubs hubs{L.hub_first.p, L.hub_nch.p, (int32_t)L.nhubs};
        {
            vgl_timed_launch tl(c, "edge_hubs");
            hipLaunchKernelGGL(vgl_k_edge_hubs_heads<BWD>, dim3(vgl_grid(L.nhubs * a.H, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, hubs, a.H, a.part);
        }
        vgl_timed_launch tl(c, "edge_hub_write");
        hipLaunchKernelGGL((vgl_k_edge_hub_write_heads<BWD, HB>), dim3(vgl_grid(L.n[VGL_RC_WG], 1, agg_grid_cap[VGL_RC_WG])), dim3(VGL_BLOCK), 0, st, list[VGL_RC_WG],
                           (int32_t)L.n[VGL_RC_WG], a);
    }
    return 0;
}

template <bool BWD>
int edge_rows_heads_run(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_x, const float *d_g, int32_t H, float *d_out, vgl_hip_agg_stats *stats)
{
    VGL_HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const vgl_agg_lists &L = p->fwd;
    edge_rows_heads_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->rowptr; a.x = d_x; a.g = d_g; a.out = d_out;
    a.chunk = L.ch.chunk; a.H = H;
    a.wide = agg_aligned16(d_x) && agg_aligned16(d_out) && (!BWD || agg_aligned16(d_g)) ? 1 : 0;
    vgl_dev<float> part;
    if (L.nhubs > 0) VGL_TRY(part.alloc(st, 2 * (size_t)L.n[VGL_RC_WG] * (size_t)H));
    a.part = reinterpret_cast<float2 *>(part.p);
    const int hb = edge_head_block(H);
    if (hb == 8) VGL_TRY((edge_rows_heads_launch<BWD, 8>(c, L, a)));
    else if (hb == 4) VGL_TRY((edge_rows_heads_launch<BWD, 4>(c, L, a)));
    else if (hb == 2) VGL_TRY((edge_rows_heads_launch<BWD, 2>(c, L, a)));
    else VGL_TRY((edge_rows_heads_launch<BWD, 1>(c, L, a)));
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // (the partials are free again; the result is there when the call returns)
    if (stats) {
        const int32_t tiles[VGL_RC_N] = {1, 1, 1};
        // per (entry, head): forward three walks of e and y written; backward two walks of y and gy and ge written; 8 bytes of bounds per row
        edge_stats(p, tiles, a.wide && hb >= 4 ? 4 : 1, 0, (int64_t)H * (BWD ? 8 * 2 + 4 : 4 * 3 + 4), 8, stats, H);
    }
    return 0;
}

// ---- the additive score of GAT and the entry sums that are its gradients ----
// e[p, h] = act(s[row(p), h] + t[adj[p], h]), act(z) = z > 0 ? z : slope * z.  Every lane is an entry slot that carries a block of HB heads, four
// entries in flight; adj[p] is read once per entry and kept across the blocks, the row's s block stays in registers where one block covers H and is
// re-read per (four entries, block) from cache otherwise (the address is the team's).  A NULL s or t is ABSENT: no addition is made, so the other
// term passes with its bits (a -0 stays -0).  No fold, no LDS, no hub stage: a chunk is an item like any other.
struct edge_add_args {
    const int64_t *rowptr;
    const int32_t *adj;
    const float *s, *t;          // n_rows x H (lds), n_cols x H (ldt); one of them may be NULL
    float *e;                    // E x H
    int64_t lds, ldt;
    int32_t H, chunk;
    float slope;
    int32_t wide_s, wide_t, wide_e;      // a lane's block of heads goes as 8- or 16-byte accesses
};

template <int HB>
__device__ __forceinline__ void edge_add_act(const edge_add_args &a, const float *sv, const float *x, float *r)
{
#pragma unroll
    for (int k = 0; k < HB; k++) {
        const float z = a.s ? (a.t ? sv[k] + x[k] : sv[k]) : x[k];
        r[k] = z > 0.0f ? z : a.slope * z;
    }
}

template <int CLS, int HB>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_add_heads(agg_list l, int32_t n, edge_add_args a)
{
    using T = vgl_rc_team<CLS>;
    const bool ws = a.wide_s != 0, wt = a.wide_t != 0, we = a.wide_e != 0, single = a.H == HB;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        int32_t v = 0;
        int64_t lo = 0, hi = 0;
        if (i < n) {
            v = l.rows[i];
            lo = a.rowptr[v]; hi = a.rowptr[v + 1];
            if constexpr (CLS == VGL_RC_WG) {
                const int64_t end = hi;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        const float *srow = a.s ? a.s + (int64_t)v * a.lds : nullptr;
        float sv[HB];
#pragma unroll
        for (int k = 0; k < HB; k++) sv[k] = 0.0f;
        if (single && srow && lo < hi) edge_load_heads<HB>(srow, ws, sv);
        int64_t p = lo + T::lane();
        for (; p + 3 * (int64_t)T::LANES < hi; p += 4 * (int64_t)T::LANES) {          // four entries in flight
            int32_t u[4] = {0, 0, 0, 0};
            if (a.t)
#pragma unroll
                for (int j = 0; j < 4; j++) u[j] = a.adj[p + j * (int64_t)T::LANES];
            for (int h0 = 0; h0 < a.H; h0 += HB) {
                if (!single && srow) edge_load_heads<HB>(srow + h0, ws, sv);
                float x[4][HB];
#pragma unroll
                for (int j = 0; j < 4; j++) {
#pragma unroll
                    for (int k = 0; k < HB; k++) x[j][k] = 0.0f;
                    if (a.t) edge_load_heads<HB>(a.t + (int64_t)u[j] * a.ldt + h0, wt, x[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float r[HB];
                    edge_add_act<HB>(a, sv, x[j], r);
                    edge_store_heads<HB>(a.e + (p + j * (int64_t)T::LANES) * a.H + h0, we, r);
                }
            }
        }
        for (; p < hi; p += T::LANES) {
            const int32_t u = a.t ? a.adj[p] : 0;
            for (int h0 = 0; h0 < a.H; h0 += HB) {
                if (!single && srow) edge_load_heads<HB>(srow + h0, ws, sv);
                float x[HB], r[HB];
#pragma unroll
                for (int k = 0; k < HB; k++) x[k] = 0.0f;
                if (a.t) edge_load_heads<HB>(a.t + (int64_t)u * a.ldt + h0, wt, x);
                edge_add_act<HB>(a, sv, x, r);
                edge_store_heads<HB>(a.e + p * a.H + h0, we, r);
            }
        }
    }
}

// out[i, h] = the sum over the entries p of row i of c(p, h), c = w[p, h], or slope * w[p, h] where GATE and gate[p, h] <= 0 (the derivative of the
// activation above, torch's: 1 for gate > 0, slope otherwise).  The walk and the fold of vgl_k_edge_rows_heads's backward sum; with TR over the
// transpose, w and gate read through the origin.  A row of one chunk is written by its team's lead lane, a chunk of a longer row leaves one float
// per (item, head) and vgl_k_edge_sum_hubs, a thread per (hub row, head), adds them in chunk order and writes the value.
struct edge_sum_args {
    const int64_t *rowptr;       // of the CSR walked
    const int32_t *origin;       // TR: the position p of each entry of the transpose
    const float *w, *gate;       // E x H
    float *out;                  // rows x H (ldo)
    float *part;                 // per (workgroup item, head)
    int64_t ldo;
    int32_t chunk, H;
    float slope;
    int32_t wide;                // w and gate are 16-byte aligned
};

template <bool GATE, int HB>
__device__ __forceinline__ void edge_sum_term(const edge_sum_args &a, int64_t o, int h0, bool wide, float *c)
{
    edge_load_heads<HB>(a.w + o * a.H + h0, wide, c);
    if constexpr (GATE) {
        float g[HB];
        edge_load_heads<HB>(a.gate + o * a.H + h0, wide, g);
#pragma unroll
        for (int k = 0; k < HB; k++) c[k] = g[k] > 0.0f ? c[k] : a.slope * c[k];
    }
}

template <int CLS, bool GATE, bool TR, int HB>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_sum_heads(agg_list l, int32_t n, edge_sum_args a)
{
    using T = vgl_rc_team<CLS>;
    const bool wide = a.wide != 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int32_t v = 0;
        int64_t lo = 0, hi = 0;
        bool whole = true;
        if (has) {
            v = l.rows[i];
            lo = a.rowptr[v]; hi = a.rowptr[v + 1];
            if constexpr (CLS == VGL_RC_WG) {
                const int64_t end = hi;
                whole = hi - lo <= a.chunk;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        const int64_t first = lo + T::lane();
        for (int h0 = 0; h0 < a.H; h0 += HB) {                         // the blocks of heads: the same trips in every lane
            float acc[HB];
#pragma unroll
            for (int k = 0; k < HB; k++) acc[k] = 0.0f;
            int64_t p = first;
            for (; p + 3 * (int64_t)T::LANES < hi; p += 4 * (int64_t)T::LANES) {      // four entries in flight, added in entry order
                int64_t o[4];
                float c[4][HB];
#pragma unroll
                for (int j = 0; j < 4; j++) o[j] = TR ? (int64_t)a.origin[p + j * (int64_t)T::LANES] : p + j * (int64_t)T::LANES;
#pragma unroll
                for (int j = 0; j < 4; j++) edge_sum_term<GATE, HB>(a, o[j], h0, wide, c[j]);
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int k = 0; k < HB; k++) acc[k] = acc[k] + c[j][k];
            }
            for (; p < hi; p += T::LANES) {
                float c[HB];
                edge_sum_term<GATE, HB>(a, TR ? (int64_t)a.origin[p] : p, h0, wide, c);
#pragma unroll
                for (int k = 0; k < HB; k++) acc[k] = acc[k] + c[k];
            }
            edge_team_sum_heads<CLS, HB>(acc);
            if (T::lead() && has) {
                float *to = CLS == VGL_RC_WG && !whole ? a.part + i * a.H + h0 : a.out + (int64_t)v * a.ldo + h0;
#pragma unroll
                for (int k = 0; k < HB; k++) to[k] = acc[k];
            }
        }
    }
}

struct edge_sum_hubs { const int32_t *row, *first, *nch; int32_t n; };
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_edge_sum_hubs(edge_sum_hubs h, int32_t H, const float *part, float *out, int64_t ldo)
{
    const int64_t total = (int64_t)h.n * H;
    for (int64_t t = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t k = (int32_t)(t / H);
        const int64_t hd = t - (int64_t)k * H;
        const float *mine = part + (int64_t)h.first[k] * H + hd;
        const int32_t nch = h.nch[k];
        float s = mine[0];
        for (int32_t j = 1; j < nch; j++) s = s + mine[(int64_t)j * H];
        out[(int64_t)h.row[k] * ldo + hd] = s;
    }
}

template <int HB>
int edge_add_launch(vgl_hip_ctx *c, const vgl_agg_lists &L, const edge_add_args &a)
{
    const char *const slot[VGL_RC_N] = {"edge_add_short", "edge_add_wave", "edge_add_wg"};
    const agg_list list[VGL_RC_N] = {{L.rows.p, nullptr}, {L.rows.p + L.n[0], nullptr}, {L.item_row.p, L.item_chunk.p}};
    return vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_add_heads<VGL_RC_SHORT, HB>, vgl_k_edge_add_heads<VGL_RC_WAVE, HB>, vgl_k_edge_add_heads<VGL_RC_WG, HB>, list, a);
}

template <bool GATE, bool TR, int HB>
int edge_sum_launch(vgl_hip_ctx *c, const vgl_agg_lists &L, const edge_sum_args &a)
{
    const char *const slot[VGL_RC_N] = {"edge_sum_short", "edge_sum_wave", "edge_sum_wg"};
    const agg_list list[VGL_RC_N] = {{L.rows.p, nullptr}, {L.rows.p + L.n[0], nullptr}, {L.item_row.p, L.item_chunk.p}};
    VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_sum_heads<VGL_RC_SHORT, GATE, TR, HB>, vgl_k_edge_sum_heads<VGL_RC_WAVE, GATE, TR, HB>,
                               vgl_k_edge_sum_heads<VGL_RC_WG, GATE, TR, HB>, list, a));
    if (L.nhubs > 0) {
        const edge_sum_hubs hubs{L.hub_row.p, L.hub_first.p, L.hub_nch.p, (int32_t)L.nhubs};
        vgl_timed_launch tl(c, "edge_sum_hubs");
        hipLaunchKernelGGL(vgl_k_edge_sum_hubs, dim3(vgl_grid(L.nhubs * a.H, VGL_BLOCK, AGG_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream, hubs, a.H, (const float *)a.part, a.out, a.ldo);
    }
    return 0;
}

template <bool GATE, bool TR>
int edge_sum_pick(vgl_hip_ctx *c, const vgl_agg_lists &L, const edge_sum_args &a)
{
    const int hb = edge_head_block(a.H);
    if (hb == 8) return edge_sum_launch<GATE, TR, 8>(c, L, a);
    if (hb == 4) return edge_sum_launch<GATE, TR, 4>(c, L, a);
    if (hb == 2) return edge_sum_launch<GATE, TR, 2>(c, L, a);
    return edge_sum_launch<GATE, TR, 1>(c, L, a);
}

// the stats of a walk over L (the plan's lists or the transpose's, `rows` rows): `per_entry` bytes per entry, `per_row` per row beside the list entries
void edge_walk_stats(const vgl_agg_lists &L, int64_t rows, int transposed, int vec, int64_t per_entry, int64_t per_row, int32_t heads, vgl_hip_agg_stats *stats)
{
    vgl_hip_agg_stats s;
    memset(&s, 0, sizeof(s));
    s.rows = rows; s.entries = L.entries;
    s.rows_short = L.rows_of[0]; s.rows_wave = L.rows_of[1]; s.rows_wg = L.rows_of[2];
    s.chunks = L.n[VGL_RC_WG]; s.hub_rows = L.nhubs;
    s.transposed = transposed; s.vec = vec; s.heads = heads;
    for (int q = 0; q < VGL_RC_N; q++) s.column_tiles[q] = 1;
    s.algorithmic_bytes = L.entries * per_entry + rows * per_row + 4 * (L.rows_of[0] + L.rows_of[1]) + 8 * L.n[VGL_RC_WG];
    *stats = s;
}

// [a, a + na) and [b, b + nb) in bytes share a byte
bool edge_overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
    if (!a || !b || na <= 0 || nb <= 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}
// the bytes from the first to the last element of a rows x H matrix of leading dimension ld
int64_t edge_span(int64_t rows, int64_t ld, int32_t H) { return rows > 0 ? 4 * ((rows - 1) * ld + H) : 0; }

}  // namespace

extern "C" {

int vgl_hip_agg_sddmm_heads(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_a, int64_t lda, const float *d_b, int64_t ldb, int32_t F, int32_t H, int mean, float *d_e,
                            vgl_hip_agg_stats *stats)
{
    // every refusal comes before the first write to an output
    VGL_TRY(edge_check_call("agg_sddmm_heads", c, p, d_a, d_b, d_e));
    if (F < 1) VGL_FAIL("agg_sddmm_heads: F must be at least 1");
    if (H < 1) VGL_FAIL("agg_sddmm_heads: H must be at least 1");
    if (F % H != 0) VGL_FAIL("agg_sddmm_heads: F must be a multiple of H");
    if (lda < F || ldb < F) VGL_FAIL("agg_sddmm_heads: a leading dimension must not be below F");
    if (mean != 0 && mean != 1) VGL_FAIL("agg_sddmm_heads: mean must be 0 or 1");
    VGL_HIP_TRY(hipSetDevice(c->device));
    const vgl_agg_lists &L = p->fwd;
    edge_dot_heads_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->rowptr; a.adj = p->adj;
    a.a = d_a; a.lda = lda; a.b = d_b; a.ldb = ldb; a.e = d_e;
    a.H = H; a.D = F / H; a.chunk = L.ch.chunk; a.mean = mean;
    const int vec = a.D % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && agg_aligned16(d_a) && agg_aligned16(d_b) ? 4 : 1;
    agg_shape(a.D, vec, a.lognq, a.tiles);
    int32_t walks[VGL_RC_N];
    for (int q = 0; q < VGL_RC_N; q++) {
        const int room = (q == VGL_RC_SHORT ? 3 : 6) - a.lognq[q];    // the lanes of a slot: 8 in the short class, 64 in the others
        int lg = 0;
        while (lg < room && ((int64_t)1 << lg) < H) lg++;
        a.loghp[q] = lg;
        a.passes[q] = (int32_t)vgl_ceil_div(H, (int64_t)1 << lg);
        walks[q] = a.passes[q] * a.tiles[q];
    }
    const char *const slot[VGL_RC_N] = {"edge_dot_short", "edge_dot_wave", "edge_dot_wg"};
    const agg_list list[VGL_RC_N] = {{L.rows.p, nullptr}, {L.rows.p + L.n[0], nullptr}, {L.item_row.p, L.item_chunk.p}};
    if (vec == 4)
        VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_dot_heads<VGL_RC_SHORT, 4>, vgl_k_edge_dot_heads<VGL_RC_WAVE, 4>, vgl_k_edge_dot_heads<VGL_RC_WG, 4>, list, a));
    else
        VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_dot_heads<VGL_RC_SHORT, 1>, vgl_k_edge_dot_heads<VGL_RC_WAVE, 1>, vgl_k_edge_dot_heads<VGL_RC_WG, 1>, list, a));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));                     // (the result is there when the call returns)
    // per entry: 4 F of b gathered and 4 H of e written; per row: the bounds and 4 F of a; the adjacency once per pass and tile (requested)
    if (stats) edge_stats(p, walks, vec, 4, 4 * (int64_t)F + 4 * (int64_t)H, 8 + 4 * (int64_t)F, stats, H);
    return 0;
}

int vgl_hip_agg_edge_softmax_heads(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_e, int32_t H, float *d_y, vgl_hip_agg_stats *stats)
{
    VGL_TRY(edge_check_call("agg_edge_softmax_heads", c, p, d_e, d_y, d_y));
    if (H < 1) VGL_FAIL("agg_edge_softmax_heads: H must be at least 1");
    return edge_rows_heads_run<false>(c, p, d_e, nullptr, H, d_y, stats);
}

int vgl_hip_agg_edge_softmax_backward_heads(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_y, const float *d_gy, int32_t H, float *d_ge, vgl_hip_agg_stats *stats)
{
    VGL_TRY(edge_check_call("agg_edge_softmax_backward_heads", c, p, d_y, d_gy, d_ge));
    if (H < 1) VGL_FAIL("agg_edge_softmax_backward_heads: H must be at least 1");
    return edge_rows_heads_run<true>(c, p, d_y, d_gy, H, d_ge, stats);
}

int vgl_hip_agg_sddmm(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_a, int64_t lda, const float *d_b, int64_t ldb, int32_t F, int mean, float *d_e, vgl_hip_agg_stats *stats)
{
    // every refusal comes before the first write to an output
    VGL_TRY(edge_check_call("agg_sddmm", c, p, d_a, d_b, d_e));
    if (F < 1) VGL_FAIL("agg_sddmm: F must be at least 1");
    if (lda < F || ldb < F) VGL_FAIL("agg_sddmm: a leading dimension must not be below F");
    if (mean != 0 && mean != 1) VGL_FAIL("agg_sddmm: mean must be 0 or 1");
    VGL_HIP_TRY(hipSetDevice(c->device));
    const vgl_agg_lists &L = p->fwd;
    edge_dot_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->rowptr; a.adj = p->adj;
    a.a = d_a; a.lda = lda; a.b = d_b; a.ldb = ldb; a.e = d_e;
    a.F = F; a.chunk = L.ch.chunk; a.mean = mean;
    const int vec = F % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && agg_aligned16(d_a) && agg_aligned16(d_b) ? 4 : 1;
    agg_shape(F, vec, a.lognq, a.tiles);
    const char *const slot[VGL_RC_N] = {"edge_dot_short", "edge_dot_wave", "edge_dot_wg"};
    const agg_list list[VGL_RC_N] = {{L.rows.p, nullptr}, {L.rows.p + L.n[0], nullptr}, {L.item_row.p, L.item_chunk.p}};
    if (vec == 4)
        VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_dot<VGL_RC_SHORT, 4>, vgl_k_edge_dot<VGL_RC_WAVE, 4>, vgl_k_edge_dot<VGL_RC_WG, 4>, list, a));
    else
        VGL_TRY(vgl_rc_launch_trio(c, slot, L.n, agg_grid_cap, vgl_k_edge_dot<VGL_RC_SHORT, 1>, vgl_k_edge_dot<VGL_RC_WAVE, 1>, vgl_k_edge_dot<VGL_RC_WG, 1>, list, a));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));                     // (the result is there when the call returns)
    // per entry: 4 F of b gathered and e written; per row: the bounds and 4 F of a; the adjacency once per column tile
    if (stats) edge_stats(p, a.tiles, vec, 4, 4 * (int64_t)F + 4, 8 + 4 * (int64_t)F, stats);
    return 0;
}

int vgl_hip_agg_edge_softmax(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_e, float *d_y, vgl_hip_agg_stats *stats)
{
    VGL_TRY(edge_check_call("agg_edge_softmax", c, p, d_e, d_y, d_y));
    return edge_rows_run<false>(c, p, d_e, nullptr, d_y, stats);
}

int vgl_hip_agg_edge_softmax_backward(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_y, const float *d_gy, float *d_ge, vgl_hip_agg_stats *stats)
{
    VGL_TRY(edge_check_call("agg_edge_softmax_backward", c, p, d_y, d_gy, d_ge));
    return edge_rows_run<true>(c, p, d_y, d_gy, d_ge, stats);
}

int vgl_hip_agg_edge_add_heads(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_s, int64_t lds, const float *d_t, int64_t ldt, int32_t H, float slope, float *d_e,
                               vgl_hip_agg_stats *stats)
{
    // every refusal comes before the first write to an output
    if (!c || !p || !d_e) VGL_FAIL("agg_edge_add_heads: null argument");
    if (!d_s && !d_t) VGL_FAIL("agg_edge_add_heads: d_s and d_t must not both be NULL");
    if (p->c != c) VGL_FAIL("agg_edge_add_heads: the plan belongs to another context");
    if (H < 1) VGL_FAIL("agg_edge_add_heads: H must be at least 1");
    if ((d_s && lds < H) || (d_t && ldt < H)) VGL_FAIL("agg_edge_add_heads: a leading dimension must not be below H");
    if (!(slope >= 0.0f) || std::isinf(slope)) VGL_FAIL("agg_edge_add_heads: slope must be finite and not negative");
    const vgl_agg_lists &L = p->fwd;
    const int64_t e_bytes = 4 * L.entries * (int64_t)H;
    if (edge_overlap(d_e, e_bytes, d_s, edge_span(p->n_rows, lds, H)) || edge_overlap(d_e, e_bytes, d_t, edge_span(p->n_cols, ldt, H)))
        VGL_FAIL("agg_edge_add_heads: d_e must not overlap d_s or d_t");
    VGL_HIP_TRY(hipSetDevice(c->device));
    edge_add_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = p->rowptr; a.adj = p->adj;
    a.s = d_s; a.lds = lds; a.t = d_t; a.ldt = ldt; a.e = d_e;
    a.H = H; a.chunk = L.ch.chunk; a.slope = slope;
    const int hb = edge_head_block(H), piece = hb >= 4 ? 4 : 2;      // a block goes in pieces of 16 bytes, a block of two heads in one of 8
    a.wide_s = d_s && agg_aligned16(d_s) && lds % piece == 0 ? 1 : 0;
    a.wide_t = d_t && agg_aligned16(d_t) && ldt % piece == 0 ? 1 : 0;
    a.wide_e = agg_aligned16(d_e) ? 1 : 0;
    if (hb == 8) VGL_TRY(edge_add_launch<8>(c, L, a));
    else if (hb == 4) VGL_TRY(edge_add_launch<4>(c, L, a));
    else if (hb == 2) VGL_TRY(edge_add_launch<2>(c, L, a));
    else VGL_TRY(edge_add_launch<1>(c, L, a));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));                     // (the result is there when the call returns)
    if (stats) {
        const bool wide = a.wide_e && (!d_s || a.wide_s) && (!d_t || a.wide_t);
        // per entry: the adjacency, 4 H of t gathered, 4 H of e written; per row: the bounds and 4 H of s
        edge_walk_stats(L, p->n_rows, 0, wide && hb >= 4 ? 4 : 1, 4 + (d_t ? 4 * (int64_t)H : 0) + 4 * (int64_t)H, 8 + (d_s ? 4 * (int64_t)H : 0), H, stats);
    }
    return 0;
}

int vgl_hip_agg_edge_sum_heads(vgl_hip_ctx *c, vgl_hip_agg_plan *p, const float *d_w, const float *d_gate, float slope, int32_t H, int transposed, float *d_out, int64_t ldo,
                               vgl_hip_agg_stats *stats)
{
    // every refusal comes before the first write to an output
    if (!c || !p || !d_w || !d_out) VGL_FAIL("agg_edge_sum_heads: null argument");
    if (p->c != c) VGL_FAIL("agg_edge_sum_heads: the plan belongs to another context");
    if (H < 1) VGL_FAIL("agg_edge_sum_heads: H must be at least 1");
    if (ldo < H) VGL_FAIL("agg_edge_sum_heads: a leading dimension must not be below H");
    if (!(slope >= 0.0f) || std::isinf(slope)) VGL_FAIL("agg_edge_sum_heads: slope must be finite and not negative");
    if (transposed != 0 && transposed != 1) VGL_FAIL("agg_edge_sum_heads: transposed must be 0 or 1");
    const int64_t rows = transposed ? p->n_cols : p->n_rows, e_bytes = 4 * p->E * (int64_t)H, out_bytes = edge_span(rows, ldo, H);
    if (edge_overlap(d_out, out_bytes, d_w, e_bytes) || edge_overlap(d_out, out_bytes, d_gate, e_bytes)) VGL_FAIL("agg_edge_sum_heads: d_out must not overlap d_w or d_gate");
    VGL_HIP_TRY(hipSetDevice(c->device));
    if (transposed && !p->has_tr) VGL_TRY(agg_build_transpose(c, p));
    hipStream_t st = c->stream;
    const vgl_agg_lists &L = transposed ? p->tr : p->fwd;
    edge_sum_args a;
    memset(&a, 0, sizeof(a));
    a.rowptr = transposed ? p->t_rowptr.p : p->rowptr;
    a.origin = transposed ? p->t_origin.p : nullptr;
    a.w = d_w; a.gate = d_gate; a.out = d_out; a.ldo = ldo;
    a.chunk = L.ch.chunk; a.H = H; a.slope = slope;
    a.wide = agg_aligned16(d_w) && (!d_gate || agg_aligned16(d_gate)) ? 1 : 0;
    vgl_dev<float> part;
    if (L.nhubs > 0) VGL_TRY(part.alloc(st, (size_t)L.n[VGL_RC_WG] * (size_t)H));
    a.part = part.p;
    if (d_gate) {
        if (transposed) VGL_TRY((edge_sum_pick<true, true>(c, L, a)));
        else VGL_TRY((edge_sum_pick<true, false>(c, L, a)));
    } else {
        if (transposed) VGL_TRY((edge_sum_pick<false, true>(c, L, a)));
        else VGL_TRY((edge_sum_pick<false, false>(c, L, a)));
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // (the partials are free again; the result is there when the call returns)
    // per entry: 4 H of w, 4 H of the gate, the origin of a transposed entry; per row: the bounds and 4 H written
    if (stats)
        edge_walk_stats(L, rows, transposed, a.wide && edge_head_block(H) >= 4 ? 4 : 1, 4 * (int64_t)H * (d_gate ? 2 : 1) + (transposed ? 4 : 0), 8 + 4 * (int64_t)H, H, stats);
    return 0;
}

}  // extern "C"
