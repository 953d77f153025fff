// vgl_agg.h -- what agg.hip (neighbour aggregation) and edge.hip (edge scores and edge softmax, section 30) share: the plan with its
// class lists and chunks, the list a team kernel runs over, the grid caps and the 16-byte load / store helpers.  The plan is built in agg.hip alone.
#pragma once
#include "vgl_rowclass.h"
#include "vgl_prim.h"

constexpr int64_t AGG_MAX_GRID = 1024;           // workgroups of a grid-stride kernel
static const int64_t agg_grid_cap[VGL_RC_N] = {4096, 4096, 4096};

#ifdef __HIPCC__
template <int VEC> __device__ __forceinline__ void agg_load(const float *p, float *out)
{
    if constexpr (VEC == 4) { const float4 t = *reinterpret_cast<const float4 *>(p); out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = t.w; }
    else out[0] = p[0];
}
template <int VEC> __device__ __forceinline__ void agg_load(const int32_t *p, int32_t *out)
{
    if constexpr (VEC == 4) { const int4 t = *reinterpret_cast<const int4 *>(p); out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = t.w; }
    else out[0] = p[0];
}
template <int VEC> __device__ __forceinline__ void agg_store(float *p, const float *v)
{
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}
template <int VEC> __device__ __forceinline__ void agg_store(int32_t *p, const int32_t *v)
{
    if constexpr (VEC == 4) *reinterpret_cast<int4 *>(p) = make_int4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}
#endif

// the items of a class: rows; the workgroup class lists chunks: item i is chunk chunk[i] of row rows[i]
struct agg_list { const int32_t *rows, *chunk; };

static inline bool agg_aligned16(const void *q) { return ((uintptr_t)q & 15u) == 0; }

// the lanes per column tile of each class, and the tiles
static inline void agg_shape(int32_t F, int vec, int32_t *lognq, int32_t *tiles)
{
    const int64_t groups = vgl_ceil_div(F, vec);
    for (int q = 0; q < VGL_RC_N; q++) {
        const int cap = q == VGL_RC_SHORT ? 3 : 6;                    // 8 lanes of a short team, 64 of a wave (the workgroup folds its four waves)
        int lg = 0;
        while (lg < cap && ((int64_t)1 << lg) < groups) lg++;
        lognq[q] = lg;
        tiles[q] = (int32_t)vgl_ceil_div(groups, (int64_t)1 << lg);
    }
}

// the rows of a CSR by class in ascending order, the chunks of its workgroup rows and the rows of more than one chunk
struct vgl_agg_lists {
    vgl_dev<int32_t> rows;                           // class 0, then 1, then 2
    vgl_dev<int32_t> item_row, item_chunk;           // the workgroup class's items: (row, chunk)
    vgl_dev<int32_t> hub_row, hub_first, hub_nch;    // the rows of more than one chunk: row, first item, chunks
    int64_t n[VGL_RC_N] = {0, 0, 0};                 // items per class
    int64_t rows_of[VGL_RC_N] = {0, 0, 0}, entries_of[VGL_RC_N] = {0, 0, 0};
    int64_t nhubs = 0, entries = 0;
    vgl_rc_chunks ch = vgl_rc_chunks::whole();
};

struct vgl_hip_agg_plan {
    vgl_hip_ctx *c = nullptr;
    const int64_t *rowptr = nullptr;                 // borrowed
    const int32_t *adj = nullptr;
    int32_t n_rows = 0, n_cols = 0;
    int64_t E = 0;
    vgl_rc_bounds b{};
    int64_t chunk_env = 0;
    vgl_agg_lists fwd, tr;
    bool has_tr = false;
    vgl_dev<int64_t> t_rowptr;                       // the transpose: n_cols rows
    vgl_dev<int32_t> t_adj, t_origin;                // row(p) and p of its entries
};

// agg.hip: builds p->tr, t_rowptr, t_adj and t_origin (the caller has made the context's device current and checks p->has_tr first)
int agg_build_transpose(vgl_hip_ctx *c, vgl_hip_agg_plan *p);
