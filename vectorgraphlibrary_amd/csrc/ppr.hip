// ppr.hip -- batched personalised PageRank of the stored directed graph by power iteration: up to 16 seed sets per pass over the incoming entries,
// float64, the damping and the stopping tolerance of the caller's choice, the dangling mass returned along the teleport vector (networkx's pagerank
// with dangling = personalization).  The contract is written out in include/vgl_hip.h; DESIGN section 28 has the kernels, their resources, the bytes
// model, the tolerance and the measurements.
//
// Per batch of width W (1, 4 or 16: the smallest that holds the batch) the state is vertex-major: x, y = x / outdeg and their successors are V x W
// float64, a vertex's W values contiguous (W = 16: one 128-byte line), so that one gather serves every column.
//   init      x = p: the dense kernel writes the uniform columns (0 elsewhere), the teleport kernel adds the listed seeds; y and the dangling mass D
//   pull      one team kernel over the row-class lists of the pull direction (short: 8 lanes per row, wave: a wavefront, wg: a workgroup per chunk
//             of VGL_PPR_CHUNK entries).  The lanes of a team are (entry slot x column pair): a lane adds the y values of its slot's entries in row
//             order, 16 bytes per load, then the slots are folded in a fixed order (xor shuffles inside a wave, LDS in wave order across a workgroup).
//             A row of more than one chunk leaves one partial per chunk; one writer adds them in chunk order (the hub kernel).
//   epilogue  the one writer of (v, column): x' = alpha * sum (+ (alpha D + 1 - alpha) / V in a uniform column), y' = x' / outdeg by one division, the
//             terms |x' - x| and (dangling v) x'.  A vertex that is a listed seed of the batch only gets x' here ...
//   teleport  ... and the rest from the teleport kernel, which touches the batch's seed vertices alone: x' += (alpha D + 1 - alpha) p[v], y', the terms.
//   fold      every workgroup of the kernels above leaves one row of 2 W partial sums (err and dangling terms per column) at its own place; one
//             workgroup adds the rows in a fixed order, leaves err and alpha D + 1 - alpha of the next iteration on the device and, when the host
//             is going to look, the largest err in the pinned mirror.
//   out       the batch transposed into the source-major d_rank.
// Every value has one writer and every sum a shape fixed by the graph, the column's place, W and the switches: no floating-point atomic, no scratch
// memory, no cooperative launch, no wait on a flag, no retry loop.  The class lists are sorted after they are filled, so the shape of the err and D
// sums does not depend on the order in which the filling kernel's appends arrived.
#include "vgl_rowclass.h"
#include "vgl_prim.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int PPR_BATCH = 16;                    // problems per batch: the widest state
constexpr int64_t PPR_MAX_GRID = 1024;           // workgroups of a grid-stride kernel
const int64_t ppr_grid_cap[VGL_RC_N] = {1024, 1024, 2048};
enum { PC_ROWS = 0, PC_TAIL = 3, PC_NCNT = 6 };
static_assert(PC_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

// how the columns of a width sit on lanes: CW columns (16 bytes where W >= 2) per lane, NQ lanes per vertex
template <int W>
struct ppr_shape {
    static constexpr int CW = W >= 2 ? 2 : 1, NQ = W / CW;
    static_assert(W == 1 || W == 4 || W == 16, "the widths of a batch");
};
template <int CW> __device__ __forceinline__ void ppr_load(const double *p, double *out)
{
    if constexpr (CW == 2) { const double2 t = *reinterpret_cast<const double2 *>(p); out[0] = t.x; out[1] = t.y; }
    else out[0] = p[0];
}
template <int CW> __device__ __forceinline__ void ppr_store(double *p, const double *v)
{
    if constexpr (CW == 2) *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]);
    else p[0] = v[0];
}

// the items of a class: rows; the workgroup class lists chunks: item i is chunk chunk[i] of row rows[i]
struct ppr_list { const int32_t *rows, *chunk; };
// one iteration
struct ppr_iter {
    const int64_t *rowptr;       // the pull direction
    const int32_t *adj;
    const int64_t *out_rowptr;   // outdeg
    const double *x, *y;         // V x W
    double *xn, *yn;
    const uint8_t *mark;         // V: the vertex is a listed seed of the batch
    const double *coef;          // W: alpha D + 1 - alpha, left by the fold before
    double *part;                // rows of 2 W: a workgroup's err terms, then its dangling terms
    double *cpart;               // W per workgroup item: the chunk sums of the rows of more than one chunk
    double alpha, inv_v;
    int32_t part_row[VGL_RC_N];  // the first partial row of the class's kernel
    int32_t chunk;               // entries per chunk
    uint32_t uniform;            // bit c: column c has the uniform p
};

// the lanes of a workgroup hold err terms e and dangling terms d of columns (lane % NQ) * CW + k: the sums over the workgroup go to one partial row.
// Lanes with equal lane % NQ are folded by an xor butterfly, the waves from LDS in wave order.  Every thread of the workgroup calls, once.
template <int NQ, int CW>
__device__ __forceinline__ void ppr_flush_terms(double *e, double *d, double *row)
{
    constexpr int W = NQ * CW;
    __shared__ double s_term[VGL_WAVES][2 * W];
#pragma unroll
    for (int k = 0; k < CW; k++)
#pragma unroll
        for (int o = NQ; o < 64; o <<= 1) {
            e[k] = e[k] + __shfl_xor(e[k], o);
            d[k] = d[k] + __shfl_xor(d[k], o);
        }
    if (vgl_lane() < NQ)
#pragma unroll
        for (int k = 0; k < CW; k++) {
            s_term[vgl_wave()][vgl_lane() * CW + k] = e[k];
            s_term[vgl_wave()][W + vgl_lane() * CW + k] = d[k];
        }
    __syncthreads();
    if (threadIdx.x < 2 * W) {
        double t = s_term[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < VGL_WAVES; w++) t = t + s_term[w][threadIdx.x];
        row[threadIdx.x] = t;
    }
}

// the one writer of columns c0 .. c0 + CW - 1 of vertex v, whose pull sums are acc
template <int W, int CW>
__device__ __forceinline__ void ppr_finish(const ppr_iter &a, int32_t v, int c0, const double *acc, double *e, double *d)
{
    const int64_t od = a.out_rowptr[v + 1] - a.out_rowptr[v], at = (int64_t)v * W + c0;
    double xv[CW], xo[CW], yv[CW];
#pragma unroll
    for (int k = 0; k < CW; k++) {
        xv[k] = a.alpha * acc[k];
        if ((a.uniform >> (c0 + k)) & 1u) xv[k] = xv[k] + a.coef[c0 + k] * a.inv_v;
    }
    ppr_store<CW>(a.xn + at, xv);
    if (a.mark[v]) return;                                            // a listed seed: the teleport kernel finishes it
    ppr_load<CW>(a.x + at, xo);
#pragma unroll
    for (int k = 0; k < CW; k++) {
        yv[k] = od > 0 ? xv[k] / (double)od : 0.0;
        e[k] = e[k] + fabs(xv[k] - xo[k]);
        if (od == 0) d[k] = d[k] + xv[k];
    }
    ppr_store<CW>(a.yn + at, yv);
}

// ---- pull: a team per row (short, wave) or per chunk (workgroup) ----
template <int CLS, int W>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_pull(ppr_list l, int32_t n, ppr_iter a)
{
    using T = vgl_rc_team<CLS>;
    constexpr int CW = ppr_shape<W>::CW, NQ = ppr_shape<W>::NQ, SLOTS = T::LANES / NQ, FOLD = T::LANES < 64 ? T::LANES : 64;
    const int q = T::lane() % NQ, slot = T::lane() / NQ;
    const double *const yq = a.y + q * CW;
    double e[CW], d[CW];
#pragma unroll
    for (int k = 0; k < CW; k++) e[k] = d[k] = 0.0;
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
                whole = end - lo <= a.chunk;
                lo += (int64_t)l.chunk[i] * a.chunk;
                hi = min(end, lo + a.chunk);
            }
        }
        double acc[CW];
#pragma unroll
        for (int k = 0; k < CW; k++) acc[k] = 0.0;
        int64_t p = lo + slot;
        for (; p + 3 * SLOTS < hi; p += 4 * SLOTS) {                  // four gathers in flight; the additions keep the row's order
            int32_t u[4];
            double t[4][CW];
#pragma unroll
            for (int j = 0; j < 4; j++) u[j] = a.adj[p + j * SLOTS];
#pragma unroll
            for (int j = 0; j < 4; j++) ppr_load<CW>(yq + (int64_t)u[j] * W, t[j]);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < CW; k++) acc[k] = acc[k] + t[j][k];
        }
        for (; p < hi; p += SLOTS) {
            double t[CW];
            ppr_load<CW>(yq + (int64_t)a.adj[p] * W, t);
#pragma unroll
            for (int k = 0; k < CW; k++) acc[k] = acc[k] + t[k];
        }
        // the slots of a column pair: an xor butterfly inside the wave, then the waves in order
#pragma unroll
        for (int k = 0; k < CW; k++)
#pragma unroll
            for (int o = NQ; o < FOLD; o <<= 1) acc[k] = acc[k] + __shfl_xor(acc[k], o);
        if constexpr (CLS == VGL_RC_WG) {
            __shared__ double s_acc[VGL_WAVES][W];
            __syncthreads();                                          // the sums of the item before have been read
            if (vgl_lane() < NQ)
#pragma unroll
                for (int k = 0; k < CW; k++) s_acc[vgl_wave()][vgl_lane() * CW + k] = acc[k];
            __syncthreads();
            if (threadIdx.x < NQ)
#pragma unroll
                for (int k = 0; k < CW; k++) {
                    double t = s_acc[0][q * CW + k];
#pragma unroll
                    for (int w = 1; w < VGL_WAVES; w++) t = t + s_acc[w][q * CW + k];
                    acc[k] = t;
                }
        }
        if (slot == 0 && has) {
            if (CLS == VGL_RC_WG && !whole) ppr_store<CW>(a.cpart + i * W + q * CW, acc);
            else ppr_finish<W, CW>(a, v, q * CW, acc, e, d);
        }
    }
    ppr_flush_terms<NQ, CW>(e, d, a.part + ((int64_t)a.part_row[CLS] + blockIdx.x) * (2 * W));
}

// the rows of more than one chunk: a thread per (row, column) adds the row's chunk sums in chunk order and finishes the vertex
struct ppr_hubs { const int32_t *row, *first, *nch; int32_t n; };
template <int W>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_hubs(ppr_hubs h, ppr_iter a, int32_t part_row)
{
    const int64_t total = (int64_t)h.n * W;
    double e[1] = {0.0}, d[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t k = (int32_t)(i / W);
        const int c = (int)(i % W);
        const double *s = a.cpart + (int64_t)h.first[k] * W + c;
        double acc[1] = {s[0]};
        for (int32_t j = 1; j < h.nch[k]; j++) acc[0] = acc[0] + s[(int64_t)j * W];
        ppr_finish<W, 1>(a, h.row[k], c, acc, e, d);
    }
    ppr_flush_terms<W, 1>(e, d, a.part + ((int64_t)part_row + blockIdx.x) * (2 * W));
}

// ---- the seed vertices of a batch: ascending, each once; p: W values per vertex (0 where the vertex is no seed of the column) ----
struct ppr_seeds { const int32_t *v; const double *p; int32_t n; };
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_mark(ppr_seeds s, uint8_t *mark, uint8_t value)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * VGL_BLOCK) mark[s.v[i]] = value;
}
// x = the uniform columns' p (0 in the others), y and the dangling terms of the vertices that are no listed seeds; coef = 1 for the teleport after it
template <int W>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_init(int32_t V, const int64_t *out_rowptr, const uint8_t *mark, uint32_t uniform, double inv_v, double *x, double *y, double *coef,
                                                            double *part)
{
    const int64_t total = (int64_t)V * W;
    double e[1] = {0.0}, d[1] = {0.0};
    if (blockIdx.x == 0 && threadIdx.x < W) coef[threadIdx.x] = 1.0;
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t v = i / W;
        const double xv = (uniform >> (int)(i % W)) & 1u ? inv_v : 0.0;
        x[i] = xv;
        if (mark[v]) continue;
        const int64_t od = out_rowptr[v + 1] - out_rowptr[v];
        y[i] = od > 0 ? xv / (double)od : 0.0;
        if (od == 0) d[0] = d[0] + xv;
    }
    ppr_flush_terms<W, 1>(e, d, part + (int64_t)blockIdx.x * (2 * W));
}
// a thread per (seed vertex, column): xn += coef * p, then what the epilogue left out.  x: the iterate before (nullptr: there is none, no err term)
template <int W>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_teleport(ppr_seeds s, const int64_t *out_rowptr, const double *x, double *xn, double *yn, const double *coef, double *part)
{
    const int64_t total = (int64_t)s.n * W;
    double e[1] = {0.0}, d[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t v = s.v[i / W];
        const int c = (int)(i % W);
        const int64_t od = out_rowptr[v + 1] - out_rowptr[v], at = (int64_t)v * W + c;
        const double xv = xn[at] + coef[c] * s.p[i];
        xn[at] = xv;
        yn[at] = od > 0 ? xv / (double)od : 0.0;
        if (x) e[0] = e[0] + fabs(xv - x[at]);
        if (od == 0) d[0] = d[0] + xv;
    }
    ppr_flush_terms<W, 1>(e, d, part + (int64_t)blockIdx.x * (2 * W));
}

// ---- fold: one workgroup adds the partial rows: value j of the rows s, s + STR, ... by thread (s, j), then the STR stripes in order ----
template <int W>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_fold(const double *part, int32_t rows, double alpha, double *coef, double *err, volatile int64_t *host, int64_t seq)
{
    constexpr int NV = 2 * W, STR = VGL_BLOCK / NV;
    __shared__ double s_sum[VGL_BLOCK];
    __shared__ double s_err[W];
    const int j = threadIdx.x % NV, s = threadIdx.x / NV;
    double t = 0.0;
    int32_t r = s;
    for (; r + 7 * STR < rows; r += 8 * STR) {                        // eight loads in flight; the additions keep the rows' order
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = part[(int64_t)(r + k * STR) * NV + j];
#pragma unroll
        for (int k = 0; k < 8; k++) t = t + v[k];
    }
    for (; r < rows; r += STR) t = t + part[(int64_t)r * NV + j];
    s_sum[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x < NV) {
        t = s_sum[threadIdx.x];
#pragma unroll
        for (int k = 1; k < STR; k++) t = t + s_sum[k * NV + threadIdx.x];
        if (threadIdx.x < W) { err[threadIdx.x] = t; s_err[threadIdx.x] = t; }
        else coef[threadIdx.x - W] = alpha * t + (1.0 - alpha);
    }
    __syncthreads();
    if (threadIdx.x == 0 && host) {
        double m = 0.0;
#pragma unroll
        for (int c = 0; c < W; c++) m = s_err[c] > m ? s_err[c] : m;
        host[0] = __double_as_longlong(m);
        __threadfence_system();
        host[C_NSLOTS] = seq;
        __threadfence_system();
    }
}

// ---- out: column c of the batch becomes row base + c of d_rank; the batch's err and iteration count ----
template <int W>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_out(int32_t V, int32_t nb, int32_t base, const double *x, double *rank, const double *err, double *d_err, int32_t *d_iterations,
                                                           int32_t iterations)
{
    constexpr int CW = ppr_shape<W>::CW;
    if (blockIdx.x == 0 && threadIdx.x < nb) {
        if (d_err) d_err[base + threadIdx.x] = err[threadIdx.x];
        if (d_iterations) d_iterations[base + threadIdx.x] = iterations;
    }
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK)
#pragma unroll
        for (int c = 0; c < W; c += CW) {
            if (c >= nb) break;
            double t[CW];
            ppr_load<CW>(x + v * W + c, t);
#pragma unroll
            for (int k = 0; k < CW; k++)
                if (c + k < nb) rank[(int64_t)(base + c + k) * V + v] = t[k];
        }
}

struct ppr_row_src {
    const int64_t *rowptr; vgl_rc_bounds b;
    __device__ __forceinline__ int cls(int64_t v, int64_t &work) const
    {
        work = rowptr[v + 1] - rowptr[v];
        return vgl_rc_class_of(work, b);
    }
};
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ppr_lengths(const int32_t *rows, int32_t n, const int64_t *rowptr, int64_t *len)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) len[i] = rowptr[rows[i] + 1] - rowptr[rows[i]];
}

}  // namespace

// what is per graph and direction, not per run, under the switches `key`: the rows by class in ascending order, the chunks of the workgroup rows and
// the rows of more than one chunk (cached on the handle, freed with it)
struct vgl_ppr_cache {
    struct dir_lists {
        vgl_dev<int32_t> rows;                       // V: class 0, then 1, then 2
        vgl_dev<int32_t> item_row, item_chunk;       // the workgroup class's items: (row, chunk)
        vgl_dev<int32_t> hub_row, hub_first, hub_nch;  // the rows of more than one chunk: row, first item, chunks
        int64_t n[VGL_RC_N] = {0, 0, 0};             // items per class
        int64_t nhubs = 0;
        bool ready = false;
    } dir[2];                                        // 0 = outgoing, 1 = incoming
    int64_t key[3] = {-1, -1, -1};
    vgl_rc_bounds b{};
    int32_t chunk = 0;
};

template <> void vgl_cache_free(vgl_ppr_cache *p) { delete p; }

namespace {

int ppr_build_dir(vgl_hip_ctx *c, vgl_hip_graph *g, vgl_ppr_cache *k, int d)
{
    hipStream_t st = c->stream;
    const vgl_dir_csr &csr = d == 0 ? g->out : g->in;
    vgl_ppr_cache::dir_lists &L = k->dir[d];
    const int32_t V = g->V;
    vgl_dev<unsigned long long> cnt;
    VGL_TRY(vgl_open_counters(c, &cnt, PC_NCNT));
    const ppr_row_src src{csr.rowptr, k->b};
    vgl_rc_lists<vgl_rc_bounded> lists;
    VGL_TRY(lists.count(c, "ppr_prepare", "ppr_prepare", src, V, PPR_MAX_GRID, cnt.p, PC_NCNT, PC_ROWS, -1, -1, V, nullptr,
                        "ppr_prepare: internal error (the row classes do not add up to the vertices)"));
    VGL_TRY(L.rows.alloc((size_t)V));
    int64_t nwg = 0;
    if (V > 0) {
        VGL_TRY(lists.fill(c, "ppr_prepare", src, V, PPR_MAX_GRID, 1, nullptr, cnt.p + PC_TAIL));
        // ascending inside a class: the order of the lists, and with it the shape of the err and D sums, is a function of the graph and the switches
        vgl_scratch tmp;
        int64_t off = 0;
        for (int q = 0; q < VGL_RC_N; q++) {
            if (lists.rows[q] > 0) {
                vgl_timed_launch tl(c, "ppr_prepare");
                VGL_TRY(vgl_sort_keys(c, tmp, (const int32_t *)lists.l[q].rows, L.rows.p + off, (size_t)lists.rows[q], 0, (unsigned)vgl_index_bits(V)));
            }
            off += lists.rows[q];
        }
        nwg = lists.rows[VGL_RC_WG];
    }
    L.n[VGL_RC_SHORT] = lists.rows[VGL_RC_SHORT];
    L.n[VGL_RC_WAVE] = lists.rows[VGL_RC_WAVE];
    // the chunks of the workgroup rows, on the host: few rows are that long
    std::vector<int32_t> rows((size_t)nwg), item_row, item_chunk, hub_row, hub_first, hub_nch;
    std::vector<int64_t> len((size_t)nwg);
    if (nwg > 0) {
        const int32_t *wg_rows = L.rows.p + lists.rows[0] + lists.rows[1];
        vgl_dev<int64_t> d_len;
        VGL_TRY(d_len.alloc(st, (size_t)nwg));
        {
            vgl_timed_launch tl(c, "ppr_prepare");
            hipLaunchKernelGGL(vgl_k_ppr_lengths, dim3(vgl_grid(nwg, VGL_BLOCK, PPR_MAX_GRID)), dim3(VGL_BLOCK), 0, st, wg_rows, (int32_t)nwg, csr.rowptr, d_len.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_HIP_TRY(hipMemcpyAsync(rows.data(), wg_rows, sizeof(int32_t) * (size_t)nwg, hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipMemcpyAsync(len.data(), d_len.p, sizeof(int64_t) * (size_t)nwg, hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
    }
    for (int64_t i = 0; i < nwg; i++) {
        if (rows[(size_t)i] < 0 || rows[(size_t)i] >= V || len[(size_t)i] <= k->b.wave) VGL_FAIL("ppr_prepare: internal error (a workgroup row is none)");
        const int64_t nch = vgl_ceil_div(len[(size_t)i], k->chunk);
        if ((int64_t)item_row.size() + nch > INT32_MAX) VGL_FAIL("ppr_prepare: the rows have more than 2^31 chunks (raise VGL_PPR_CHUNK)");
        if (nch > 1) {
            hub_row.push_back(rows[(size_t)i]);
            hub_first.push_back((int32_t)item_row.size());
            hub_nch.push_back((int32_t)nch);
        }
        for (int64_t j = 0; j < nch; j++) {
            item_row.push_back(rows[(size_t)i]);
            item_chunk.push_back((int32_t)j);
        }
    }
    L.n[VGL_RC_WG] = (int64_t)item_row.size();
    L.nhubs = (int64_t)hub_row.size();
    auto up = [&](vgl_dev<int32_t> &to, const std::vector<int32_t> &from) -> int {
        VGL_TRY(to.alloc(from.size()));
        if (!from.empty()) VGL_HIP_TRY(hipMemcpyAsync(to.p, from.data(), sizeof(int32_t) * from.size(), hipMemcpyHostToDevice, st));
        return 0;
    };
    VGL_TRY(up(L.item_row, item_row));
    VGL_TRY(up(L.item_chunk, item_chunk));
    VGL_TRY(up(L.hub_row, hub_row));
    VGL_TRY(up(L.hub_first, hub_first));
    VGL_TRY(up(L.hub_nch, hub_nch));
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // (the host vectors and the unsorted lists are free again)
    L.ready = true;
    return 0;
}

// the direction the pull walks: the incoming CSR, or the outgoing one of a graph its caller calls symmetric
int ppr_validate(const char *who, vgl_hip_ctx *c, vgl_hip_graph *g, int symmetric, int *dir)
{
    static thread_local std::string msg;
    if (!c || !g) { msg = std::string(who) + ": null argument"; VGL_FAIL(msg.c_str()); }
    if (g->row_begin != 0 || g->row_end != g->V) { msg = std::string(who) + ": graph handle must own all rows (personalised PageRank has no sharded form)"; VGL_FAIL(msg.c_str()); }
    if (!symmetric && !g->in.rowptr) {
        msg = std::string(who) + ": the pull needs the incoming CSR, or symmetric = 1 from a caller who vouches that the stored graph is symmetric";
        VGL_FAIL(msg.c_str());
    }
    *dir = symmetric ? 0 : 1;
    return 0;
}

int ppr_ensure(vgl_hip_ctx *c, vgl_hip_graph *g, int dir, vgl_ppr_cache **out, bool *built)
{
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_PPR_SHORT", "VGL_PPR_WAVE");
    const int64_t chunk = vgl_env_int(c, "VGL_PPR_CHUNK", 16384, 16, 1 << 28);
    const int64_t key[3] = {b.shrt, b.wave, chunk};
    *built = false;
    if (!g->ppr) g->ppr.reset(new vgl_ppr_cache());
    vgl_ppr_cache *k = g->ppr.get();
    if (!std::equal(key, key + 3, k->key)) {
        VGL_HIP_TRY(hipStreamSynchronize(c->stream));               // (kernels of an earlier run may still read the lists)
        k->dir[0].ready = k->dir[1].ready = false;
        k->b = b;
        k->chunk = (int32_t)chunk;
        std::copy(key, key + 3, k->key);
    }
    if (!k->dir[dir].ready) {
        VGL_TRY(ppr_build_dir(c, g, k, dir));
        *built = true;
    }
    *out = k;
    return 0;
}

// what a batch needs of its call
struct ppr_run {
    vgl_hip_ctx *c;
    vgl_hip_graph *g;
    const vgl_dir_csr *csr;
    const vgl_ppr_cache::dir_lists *L;
    int32_t chunk;
    double alpha, tol;
    int32_t max_iterations;
    double *state[4];            // x, y, and their successors: V x 16 each
    uint8_t *mark;
    double *coef, *err, *part, *cpart;
    double *d_rank, *d_err;
    int32_t *d_iterations;
};

// One batch of nb problems at base: seeds (device, with p of width W) are its distinct listed seed vertices, uniform the columns of the uniform p.
// *iterations = what it ran, *max_err = the largest err of its last iteration, *converged = the tolerance stopped it.
template <int W>
int ppr_batch(const ppr_run &r, int32_t base, int32_t nb, ppr_seeds seeds, uint32_t uniform, int32_t *iterations, double *max_err, bool *converged)
{
    vgl_hip_ctx *c = r.c;
    hipStream_t st = c->stream;
    const int32_t V = r.g->V;
    const int64_t *out_rowptr = r.g->out.rowptr;
    const double inv_v = 1.0 / (double)V;
    double *x = r.state[0], *y = r.state[1], *xn = r.state[2], *yn = r.state[3];
    const unsigned grid_seeds = vgl_grid((int64_t)seeds.n * W, VGL_BLOCK, PPR_MAX_GRID), grid_init = vgl_grid((int64_t)V * W, VGL_BLOCK, PPR_MAX_GRID);
    auto fold = [&](int32_t rows, bool look) -> int {
        const int64_t seq = look ? vgl_next_seq(c) : 0;
        {
            vgl_timed_launch tl(c, "ppr_fold");
            hipLaunchKernelGGL(vgl_k_ppr_fold<W>, dim3(1), dim3(VGL_BLOCK), 0, st, (const double *)r.part, rows, r.alpha, r.coef, r.err, look ? (volatile int64_t *)c->h_counters : nullptr, seq);
        }
        VGL_HIP_TRY(hipGetLastError());
        if (look) {
            VGL_TRY(vgl_wait_counters(c, seq));
            memcpy(max_err, &c->h_counters[0], sizeof(double));
        }
        return 0;
    };
    // x = p
    {
        vgl_timed_launch tl(c, "ppr_teleport");
        if (seeds.n > 0) hipLaunchKernelGGL(vgl_k_ppr_mark, dim3(vgl_grid(seeds.n, VGL_BLOCK, PPR_MAX_GRID)), dim3(VGL_BLOCK), 0, st, seeds, r.mark, (uint8_t)1);
        hipLaunchKernelGGL(vgl_k_ppr_init<W>, dim3(grid_init), dim3(VGL_BLOCK), 0, st, V, out_rowptr, (const uint8_t *)r.mark, uniform, inv_v, x, y, r.coef, r.part);
        if (seeds.n > 0)
            hipLaunchKernelGGL(vgl_k_ppr_teleport<W>, dim3(grid_seeds), dim3(VGL_BLOCK), 0, st, seeds, out_rowptr, (const double *)nullptr, x, y, (const double *)r.coef,
                               r.part + (int64_t)grid_init * (2 * W));
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(fold((int32_t)(grid_init + (seeds.n > 0 ? grid_seeds : 0)), r.max_iterations == 0));
    // the iterations
    const char *const slot[VGL_RC_N] = {"ppr_pull_short", "ppr_pull_wave", "ppr_pull_wg"};
    const int64_t per_wg[VGL_RC_N] = {VGL_BLOCK / VGL_RC_G, VGL_WAVES, 1};
    const ppr_list list[VGL_RC_N] = {{r.L->rows.p, nullptr}, {r.L->rows.p + r.L->n[0], nullptr}, {r.L->item_row.p, r.L->item_chunk.p}};
    const ppr_hubs hubs{r.L->hub_row.p, r.L->hub_first.p, r.L->hub_nch.p, (int32_t)r.L->nhubs};
    const unsigned grid_hubs = vgl_grid(r.L->nhubs * W, VGL_BLOCK, PPR_MAX_GRID);
    ppr_iter a;
    a.rowptr = r.csr->rowptr; a.adj = r.csr->adj; a.out_rowptr = out_rowptr;
    a.mark = r.mark; a.coef = r.coef; a.part = r.part; a.cpart = r.cpart;
    a.alpha = r.alpha; a.inv_v = inv_v; a.chunk = r.chunk; a.uniform = uniform;
    int32_t rows = 0;
    for (int q = 0; q < VGL_RC_N; q++) {
        a.part_row[q] = rows;
        if (r.L->n[q] > 0) rows += (int32_t)vgl_grid(r.L->n[q], per_wg[q], ppr_grid_cap[q]);
    }
    const int32_t hub_row0 = rows;
    if (r.L->nhubs > 0) rows += (int32_t)grid_hubs;
    const int32_t seed_row0 = rows;
    if (seeds.n > 0) rows += (int32_t)grid_seeds;
    int32_t t = 0;
    *converged = false;
    while (t < r.max_iterations) {
        a.x = x; a.y = y; a.xn = xn; a.yn = yn;
        VGL_TRY(vgl_rc_launch_trio(c, slot, r.L->n, ppr_grid_cap, vgl_k_ppr_pull<VGL_RC_SHORT, W>, vgl_k_ppr_pull<VGL_RC_WAVE, W>, vgl_k_ppr_pull<VGL_RC_WG, W>, list, a));
        if (r.L->nhubs > 0) {
            vgl_timed_launch tl(c, "ppr_pull_wg");
            hipLaunchKernelGGL(vgl_k_ppr_hubs<W>, dim3(grid_hubs), dim3(VGL_BLOCK), 0, st, hubs, a, hub_row0);
        }
        if (seeds.n > 0) {
            vgl_timed_launch tl(c, "ppr_teleport");
            hipLaunchKernelGGL(vgl_k_ppr_teleport<W>, dim3(grid_seeds), dim3(VGL_BLOCK), 0, st, seeds, out_rowptr, (const double *)x, xn, yn, (const double *)r.coef,
                               r.part + (int64_t)seed_row0 * (2 * W));
        }
        VGL_HIP_TRY(hipGetLastError());
        t++;
        const bool look = r.tol > 0.0 || t == r.max_iterations;
        VGL_TRY(fold(rows, look));
        std::swap(x, xn);
        std::swap(y, yn);
        if (r.tol > 0.0 && *max_err <= r.tol) { *converged = true; break; }
    }
    *iterations = t;
    {
        vgl_timed_launch tl(c, "ppr_out");
        hipLaunchKernelGGL(vgl_k_ppr_out<W>, dim3(vgl_grid(V, VGL_BLOCK, PPR_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, nb, base, (const double *)x, r.d_rank, (const double *)r.err, r.d_err,
                           r.d_iterations, t);
    }
    if (seeds.n > 0) {
        vgl_timed_launch tl(c, "ppr_teleport");
        hipLaunchKernelGGL(vgl_k_ppr_mark, dim3(vgl_grid(seeds.n, VGL_BLOCK, PPR_MAX_GRID)), dim3(VGL_BLOCK), 0, st, seeds, r.mark, (uint8_t)0);
    }
    VGL_HIP_TRY(hipGetLastError());
    return 0;
}

// the partial rows a batch may write: every kernel of an iteration (the three classes, the hubs, the teleport) leaves one per workgroup
int64_t ppr_part_rows() { return ppr_grid_cap[0] + ppr_grid_cap[1] + ppr_grid_cap[2] + 2 * PPR_MAX_GRID; }

}  // namespace

extern "C" {

int vgl_hip_ppr_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int symmetric)
{
    int dir = 0;
    VGL_TRY(ppr_validate("ppr_prepare", c, g, symmetric, &dir));
    vgl_ppr_cache *k = nullptr;
    bool built = false;
    VGL_TRY(ppr_ensure(c, g, dir, &k, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_ppr_run(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *seeds, const int64_t *seed_ptr, const double *seed_weight, int32_t count, double alpha, int32_t max_iterations,
                    double tol, int symmetric, double *d_rank, double *d_err, int32_t *d_iterations, vgl_hip_ppr_stats *stats)
{
    // every refusal comes before the first write to an output
    int dir = 0;
    VGL_TRY(ppr_validate("ppr_run", c, g, symmetric, &dir));
    if (!std::isfinite(alpha) || alpha < 0.0 || alpha >= 1.0) VGL_FAIL("ppr_run: alpha must be finite and in [0, 1)");
    if (!std::isfinite(tol) || tol < 0.0) VGL_FAIL("ppr_run: tol must be finite and not negative");
    if (max_iterations < 0) VGL_FAIL("ppr_run: max_iterations must not be negative");
    if (count < 0) VGL_FAIL("ppr_run: count must not be negative");
    if (!d_rank) VGL_FAIL("ppr_run: d_rank must not be NULL");
    if (count > 0 && !seed_ptr) VGL_FAIL("ppr_run: seed_ptr must not be NULL");
    const int32_t V = g->V;
    if (count > 0) {
        if (seed_ptr[0] < 0) VGL_FAIL("ppr_run: seed_ptr must not decrease (it starts below 0)");
        for (int32_t j = 0; j < count; j++)
            if (seed_ptr[j + 1] < seed_ptr[j]) VGL_FAIL("ppr_run: seed_ptr must not decrease");
        if (seed_ptr[count] > seed_ptr[0] && !seeds) VGL_FAIL("ppr_run: seeds must not be NULL");
        for (int64_t i = seed_ptr[0]; i < seed_ptr[count]; i++) {
            if (seeds[i] < 0 || seeds[i] >= V) VGL_FAIL("ppr_run: seed vertex out of range");
            if (seed_weight && !(std::isfinite(seed_weight[i]) && seed_weight[i] > 0.0)) VGL_FAIL("ppr_run: a seed weight must be finite and greater than 0");
        }
        if (V == 0) VGL_FAIL("ppr_run: the graph has no vertices");
    }
    vgl_ppr_cache *k = nullptr;
    bool built = false;
    VGL_TRY(ppr_ensure(c, g, dir, &k, &built));
    hipStream_t st = c->stream;
    vgl_hip_ppr_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    if (count == 0) {
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (stats) *stats = out;
        return 0;
    }
    const vgl_dir_csr &csr = dir == 0 ? g->out : g->in;
    const vgl_ppr_cache::dir_lists &L = k->dir[dir];
    const int64_t E = csr.edges;

    // ---- scratch of the call, all of it drawn before the first batch ----
    const int wmax = count == 1 ? 1 : count <= 4 ? 4 : PPR_BATCH;
    vgl_dev<double> state[4], coef, err, part, cpart, sp;
    vgl_dev<uint8_t> mark;
    vgl_dev<int32_t> sv;
    for (int i = 0; i < 4; i++) VGL_TRY(state[i].alloc(st, (size_t)V * (size_t)wmax));
    VGL_TRY(coef.alloc(st, PPR_BATCH));
    VGL_TRY(err.alloc(st, PPR_BATCH));
    VGL_TRY(part.alloc(st, (size_t)ppr_part_rows() * 2 * PPR_BATCH));
    VGL_TRY(cpart.alloc(st, (size_t)std::max<int64_t>(L.n[VGL_RC_WG], 1) * PPR_BATCH));
    VGL_TRY(mark.alloc(st, (size_t)V));
    VGL_HIP_TRY(hipMemsetAsync(mark.p, 0, (size_t)V, st));
    size_t seed_cap = 0;
    ppr_run r;
    r.c = c; r.g = g; r.csr = &csr; r.L = &L; r.chunk = k->chunk;
    r.alpha = alpha; r.tol = tol; r.max_iterations = max_iterations;
    for (int i = 0; i < 4; i++) r.state[i] = state[i].p;
    r.mark = mark.p; r.coef = coef.p; r.err = err.p; r.part = part.p; r.cpart = cpart.p;
    r.d_rank = d_rank; r.d_err = d_err; r.d_iterations = d_iterations;

    std::vector<int32_t> h_sv;
    std::vector<double> h_sp;
    for (int32_t base = 0; base < count; base += PPR_BATCH) {
        const int32_t nb = std::min<int32_t>(PPR_BATCH, count - base);
        const int W = nb == 1 ? 1 : nb <= 4 ? 4 : PPR_BATCH;
        // p of the listed columns: the distinct seed vertices in ascending order, a row of W values each, added in list order
        uint32_t uniform = 0;
        h_sv.clear();
        for (int32_t j = 0; j < nb; j++) {
            const int64_t s0 = seed_ptr[base + j], s1 = seed_ptr[base + j + 1];
            if (s0 == s1) uniform |= 1u << j;
            h_sv.insert(h_sv.end(), seeds + s0, seeds + s1);
        }
        std::sort(h_sv.begin(), h_sv.end());
        h_sv.erase(std::unique(h_sv.begin(), h_sv.end()), h_sv.end());
        h_sp.assign(h_sv.size() * (size_t)W, 0.0);
        for (int32_t j = 0; j < nb; j++) {
            const int64_t s0 = seed_ptr[base + j], s1 = seed_ptr[base + j + 1];
            double sum = 0.0;
            for (int64_t i = s0; i < s1; i++) sum = sum + (seed_weight ? seed_weight[i] : 1.0);
            for (int64_t i = s0; i < s1; i++) {
                const size_t at = (size_t)(std::lower_bound(h_sv.begin(), h_sv.end(), seeds[i]) - h_sv.begin());
                h_sp[at * (size_t)W + (size_t)j] = h_sp[at * (size_t)W + (size_t)j] + (seed_weight ? seed_weight[i] : 1.0) / sum;
            }
        }
        if (h_sv.size() > seed_cap) {
            seed_cap = h_sv.size();
            VGL_TRY(sv.alloc(st, seed_cap));
            VGL_TRY(sp.alloc(st, seed_cap * PPR_BATCH));
        }
        if (!h_sv.empty()) {
            VGL_HIP_TRY(hipMemcpyAsync(sv.p, h_sv.data(), sizeof(int32_t) * h_sv.size(), hipMemcpyHostToDevice, st));
            VGL_HIP_TRY(hipMemcpyAsync(sp.p, h_sp.data(), sizeof(double) * h_sp.size(), hipMemcpyHostToDevice, st));
            VGL_HIP_TRY(hipStreamSynchronize(st));                    // (the host vectors are free again)
        }
        const ppr_seeds sd{sv.p, sp.p, (int32_t)h_sv.size()};
        int32_t it = 0;
        double max_err = 0.0;
        bool conv = false;
        if (W == 1) VGL_TRY(ppr_batch<1>(r, base, nb, sd, uniform, &it, &max_err, &conv));
        else if (W == 4) VGL_TRY(ppr_batch<4>(r, base, nb, sd, uniform, &it, &max_err, &conv));
        else VGL_TRY(ppr_batch<16>(r, base, nb, sd, uniform, &it, &max_err, &conv));
        out.batches++;
        out.sources += nb;
        out.iterations_total += it;
        out.iterations_max = std::max(out.iterations_max, it);
        out.batches_converged += conv ? 1 : 0;
        out.entries_walked += (int64_t)it * E;
        out.max_err = std::max(out.max_err, max_err);
        // the model (include/vgl_hip.h has the terms)
        out.algorithmic_bytes += (16 * (int64_t)W + 9) * V + (int64_t)it * (E * (4 + 8 * (int64_t)W) + (int64_t)V * (21 + 24 * (int64_t)W)) + 8 * (int64_t)V * (W + nb);
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
