// bc.hip -- betweenness centrality (Brandes) of the stored directed, unweighted graph from a set of sources.  The contract is written out in
// include/vgl_hip.h; DESIGN section 14 has the schedule, the kernel resources and the bytes model.
//
// Per source s:
//   levels   vgl_hip_bfs_run (direction-optimising when the incoming CSR exists), exactly as a caller of the BFS gets them: source 1, unreached -1.
//   order    the reached vertices bucketed by (level, row class): a histogram over the keys (per-workgroup LDS histograms folded with one atomic per
//            bucket; plain global atomics when a traversal is deeper than the LDS table), an exclusive scan on the device, the counts copied to the
//            host once (the launch ranges), a scatter with per-workgroup reservations.  One order per sweep direction (one when symmetric).  The
//            position of a vertex inside its bucket depends on arrival order; no VALUE does (below).
//   forward  level 2 .. D+1: sigma[v] = sum over v's entries in the forward CSR (incoming, or outgoing when symmetric) whose endpoint is one level up.
//   backward level D .. 1:   sum over v's outgoing entries one level down of coef[w] = (1 + delta[w]) / sigma[w]; delta[v] = sigma[v] * sum;
//            coef[v] is written for the level above; bc[v] += delta[v] for v != s in the same kernel.  The last level has delta = 0, coef = 1 / sigma.
// Both sweeps are pulls: every sigma / coef / bc entry has ONE writer per source and the summation shape of a row is fixed by its length and its class
// (lane-strided partial sums, unrolled by four in a fixed order, xor-shuffle tree, LDS fold in wave order, hub chunks in chunk order), so the result
// is bit-identical from run to run.  There are no floating-point atomics; the integer atomics only count.
// Row classes (per direction, a property of the graph, cached on the handle): short (<= VGL_BC_SHORT entries: 8 lanes per row), wave (<= VGL_BC_WAVE:
// one wavefront), workgroup (<= VGL_BC_WG: 256 threads), hub (longer: one workgroup per VGL_BC_CHUNK entries, partial sums folded in chunk order by
// a second kernel).  Every (level, class) pair is one contiguous range of the order and one launch (two for hubs).
#include "vgl_hip_internal.h"
#include "vgl_chunks.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int BC_NCLS = 4;
enum { BC_SHORT = 0, BC_WAVE = 1, BC_WG = 2, BC_HUB = 3 };
constexpr int BC_G = 8;                         // lanes per short row
constexpr int BC_LDS_BUCKETS = 4096;            // (level, class) buckets a workgroup histograms in LDS: 1024 levels
constexpr int BC_ORDER_BLOCKS = 1024;           // workgroups of the count / scatter kernels: one contiguous vertex range each
constexpr double BC_TWO53 = 9007199254740992.0;
enum { BC_C_FWD = 0, BC_C_BWD = 1, BC_C_OVERFLOW = 2, BC_NCNT = 3 };

struct bc_bounds { int32_t shrt, wave, wg; };
__host__ __device__ inline int bc_class_of(int64_t d, bc_bounds b) { return d <= b.shrt ? BC_SHORT : d <= b.wave ? BC_WAVE : d <= b.wg ? BC_WG : BC_HUB; }


// ---- prepare: the class of every row of one direction, the class sizes and the longest row ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_classify(int32_t V, const int64_t *rowptr, bc_bounds b, uint8_t *cls, int32_t *sizes, unsigned long long *max_row)
{
    __shared__ int s_n[BC_NCLS];
    if (threadIdx.x < BC_NCLS) s_n[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long m = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t d = rowptr[v + 1] - rowptr[v];
        const int k = bc_class_of(d, b);
        cls[v] = (uint8_t)k;
        atomicAdd(&s_n[k], 1);
        m = max(m, (unsigned long long)max(d, (int64_t)0));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned long long)__shfl_xor((long long)m, o));
    if (vgl_lane() == 0 && m) atomicMax(max_row, m);
    __syncthreads();
    if (threadIdx.x < BC_NCLS && s_n[threadIdx.x]) atomicAdd(sizes + threadIdx.x, s_n[threadIdx.x]);
}

// ---- order: reached vertices by (level, class) ----
// workgroup b owns the vertices [b * per, (b + 1) * per); bucket of v = (levels[v] - 1) * BC_NCLS + cls[v]; a level beyond level_cap raises the flag
template <bool LDS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_count(int32_t V, int32_t per, const int32_t *levels, const uint8_t *cls, int32_t level_cap, int32_t *hist, int64_t *cnt)
{
    __shared__ int s_h[LDS ? BC_LDS_BUCKETS : 1];
    const int nb = level_cap * BC_NCLS;
    const int64_t v0 = (int64_t)blockIdx.x * per, v1 = min((int64_t)V, v0 + per);
    if (LDS) {
        for (int i = threadIdx.x; i < nb; i += VGL_BLOCK) s_h[i] = 0;
        __syncthreads();
    }
    for (int64_t v = v0 + threadIdx.x; v < v1; v += VGL_BLOCK) {
        const int32_t l = levels[v];
        if (l <= 0) continue;
        if (l > level_cap) { vgl_atomic_add64(cnt + BC_C_OVERFLOW, 1); continue; }
        const int key = (l - 1) * BC_NCLS + cls[v];
        if (LDS) atomicAdd(&s_h[key], 1); else atomicAdd(hist + key, 1);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += VGL_BLOCK)
            if (s_h[i]) atomicAdd(hist + i, s_h[i]);
    }
}
// cursor[i] = hist[0] + .. + hist[i - 1] (one workgroup)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_scan(int32_t nb, const int32_t *hist, int32_t *cursor)
{
    __shared__ int s_w[VGL_WAVES];
    int carry = 0;
    for (int base = 0; base < nb; base += VGL_BLOCK) {       // (uniform over the workgroup)
        const int i = base + threadIdx.x;
        const int x = i < nb ? hist[i] : 0;
        int total = 0;
        const int ex = vgl_block_excl_add(x, s_w, &total);
        if (i < nb) cursor[i] = carry + ex;
        carry += total;
    }
}
// the scatter; cursor holds the bucket starts and is advanced by whole workgroup reservations.  rp_fwd / rp_bwd (either may be NULL): the sweeps'
// entry counts -- rows of the forward CSR of the reached non-source vertices, rows of the outgoing CSR of the vertices above the last level.
template <bool LDS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_scatter(int32_t V, int32_t per, const int32_t *levels, const uint8_t *cls, int32_t level_cap, int32_t *cursor,
                                                               int32_t *order, const int64_t *rp_fwd, const int64_t *rp_bwd, int32_t last_level, int64_t *cnt)
{
    __shared__ int s_h[LDS ? BC_LDS_BUCKETS : 1], s_base[LDS ? BC_LDS_BUCKETS : 1];
    __shared__ int64_t s_red[VGL_WAVES];
    const int nb = level_cap * BC_NCLS;
    const int64_t v0 = (int64_t)blockIdx.x * per, v1 = min((int64_t)V, v0 + per);
    int64_t ef = 0, eb = 0;
    if (LDS) {
        for (int i = threadIdx.x; i < nb; i += VGL_BLOCK) s_h[i] = 0;
        __syncthreads();
        for (int64_t v = v0 + threadIdx.x; v < v1; v += VGL_BLOCK) {
            const int32_t l = levels[v];
            if (l > 0 && l <= level_cap) atomicAdd(&s_h[(l - 1) * BC_NCLS + cls[v]], 1);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += VGL_BLOCK) {
            const int n = s_h[i];
            s_base[i] = n ? atomicAdd(cursor + i, n) : 0;
            s_h[i] = 0;
        }
        __syncthreads();
    }
    for (int64_t v = v0 + threadIdx.x; v < v1; v += VGL_BLOCK) {
        const int32_t l = levels[v];
        if (l <= 0 || l > level_cap) continue;
        const int key = (l - 1) * BC_NCLS + cls[v];
        const int pos = LDS ? s_base[key] + atomicAdd(&s_h[key], 1) : atomicAdd(cursor + key, 1);
        if (pos >= 0 && pos < V) order[pos] = (int32_t)v;
        if (rp_fwd && l > 1) ef += rp_fwd[v + 1] - rp_fwd[v];
        if (rp_bwd && l < last_level) eb += rp_bwd[v + 1] - rp_bwd[v];
    }
    ef = vgl_block_reduce_add(ef, s_red);
    eb = vgl_block_reduce_add(eb, s_red);
    if (threadIdx.x == 0) {
        if (ef) vgl_atomic_add64(cnt + BC_C_FWD, ef);
        if (eb) vgl_atomic_add64(cnt + BC_C_BWD, eb);
    }
}

// ---- the sweeps ----
struct bc_sweep {
    const int64_t *rowptr;       // the CSR the sweep pulls over
    const int32_t *adj;
    const int32_t *levels;
    const int32_t *order;        // the rows of this launch: order[0 .. n)
    int32_t n;
    int32_t want;                // an entry counts when its endpoint has this level
    const double *gather;        // forward: sigma; backward: coef
    double *sigma;               // forward writes it, backward reads it
    double *coef, *bc, *delta_out;      // backward only (delta_out may be NULL)
    int32_t source;
    int32_t *inexact;            // forward: set when a sigma reaches 2^53
    double *partial;             // hub kernels: n * ch.nchunks chunk sums
    vgl_rc_chunks ch;
};

// lane `lane` of `stride` lanes: its share of the entries [lo, hi), four entries in flight, added in entry order
__device__ __forceinline__ double bc_row_sum(const bc_sweep &a, int64_t lo, int64_t hi, int lane, int stride)
{
    double acc = 0.0;
    int64_t e = lo + lane;
    for (; e + 3 * (int64_t)stride < hi; e += 4 * (int64_t)stride) {
        const int32_t u0 = a.adj[e], u1 = a.adj[e + stride], u2 = a.adj[e + 2 * (int64_t)stride], u3 = a.adj[e + 3 * (int64_t)stride];
        const int32_t l0 = a.levels[u0], l1 = a.levels[u1], l2 = a.levels[u2], l3 = a.levels[u3];
        const double x0 = l0 == a.want ? a.gather[u0] : 0.0;
        const double x1 = l1 == a.want ? a.gather[u1] : 0.0;
        const double x2 = l2 == a.want ? a.gather[u2] : 0.0;
        const double x3 = l3 == a.want ? a.gather[u3] : 0.0;
        acc += x0; acc += x1; acc += x2; acc += x3;
    }
    for (; e < hi; e += stride) {
        const int32_t u = a.adj[e];
        if (a.levels[u] == a.want) acc += a.gather[u];
    }
    return acc;
}

template <bool FWD>
__device__ __forceinline__ void bc_finish(const bc_sweep &a, int32_t v, double sum)
{
    if (FWD) {
        a.sigma[v] = sum;
        if (sum >= BC_TWO53) atomicOr(a.inexact, 1);
    } else {
        const double sg = a.sigma[v];
        const double d = sg * sum;
        a.coef[v] = (1.0 + d) / sg;
        if (v != a.source) a.bc[v] += d;
        if (a.delta_out) a.delta_out[v] = d;
    }
}

template <bool FWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_short(bc_sweep a)
{
    const int64_t i = ((int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x) / BC_G;
    const int gi = threadIdx.x & (BC_G - 1);
    int32_t v = -1;
    double sum = 0.0;
    if (i < a.n) {
        v = a.order[i];
        sum = bc_row_sum(a, a.rowptr[v], a.rowptr[v + 1], gi, BC_G);
    }
#pragma unroll
    for (int o = BC_G / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (v >= 0 && gi == 0) bc_finish<FWD>(a, v, sum);
}

template <bool FWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_wave(bc_sweep a)
{
    const int64_t i = (int64_t)blockIdx.x * VGL_WAVES + vgl_wave();
    if (i >= a.n) return;                                     // (uniform over the wave)
    const int32_t v = a.order[i];
    const double sum = vgl_wave_reduce_add(bc_row_sum(a, a.rowptr[v], a.rowptr[v + 1], vgl_lane(), 64));
    if (vgl_lane() == 0) bc_finish<FWD>(a, v, sum);
}

template <bool FWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_wg(bc_sweep a)
{
    __shared__ double s_red[VGL_WAVES];
    const int32_t v = a.order[blockIdx.x];                    // grid = n
    const double sum = vgl_block_reduce_add(bc_row_sum(a, a.rowptr[v], a.rowptr[v + 1], (int)threadIdx.x, VGL_BLOCK), s_red);
    if (threadIdx.x == 0) bc_finish<FWD>(a, v, sum);
}

// hub rows: workgroup (i, k) sums chunk k of row order[i] into partial[i * nchunks + k]; grid = (n, nchunks)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_hub(bc_sweep a)
{
    __shared__ double s_red[VGL_WAVES];
    const int32_t v = a.order[blockIdx.x];
    int64_t lo, hi;
    if (!a.ch.range(a.rowptr[v], a.rowptr[v + 1], blockIdx.y, &lo, &hi)) return;      // (uniform over the workgroup)
    const double sum = vgl_block_reduce_add(bc_row_sum(a, lo, hi, (int)threadIdx.x, VGL_BLOCK), s_red);
    if (threadIdx.x == 0) a.partial[(int64_t)blockIdx.x * a.ch.nchunks + blockIdx.y] = sum;
}
// ... and one thread per hub row folds its chunk sums in chunk order
template <bool FWD>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_hub_fold(bc_sweep a)
{
    const int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int32_t v = a.order[i];
    const int64_t chunks = a.ch.pieces(a.rowptr[v + 1] - a.rowptr[v]);
    double sum = 0.0;
    for (int64_t k = 0; k < chunks; k++) sum += a.partial[i * a.ch.nchunks + k];
    bc_finish<FWD>(a, v, sum);
}

// the last level of the backward sweep: delta = 0 (delta_out was cleared), coef = 1 / sigma
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bc_leaf(const int32_t *order, int32_t n, const double *sigma, double *coef)
{
    const int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t v = order[i];
    coef[v] = 1.0 / sigma[v];
}
__global__ void vgl_k_bc_seed(double *sigma, int32_t source) { sigma[source] = 1.0; }

unsigned bc_grid(int64_t work, int64_t per_block) { return (unsigned)std::max<int64_t>(1, vgl_ceil_div(work, per_block)); }

}  // namespace

// what is per graph and not per source: the row classes of both directions under the switches `key` (cached on the handle, freed with it)
struct vgl_bc_cache {
    struct dir_classes {
        vgl_dev<uint8_t> cls;                        // V
        int32_t size[BC_NCLS] = {};
        int64_t max_row = 0;
        bool ready = false;
    } dir[2];                                        // 0 = outgoing, 1 = incoming
    int64_t key[4] = {-1, -1, -1, -1};
    bc_bounds b{};
    int32_t chunk = 0;
};

template <> void vgl_cache_free(vgl_bc_cache *p) { delete p; }

namespace {

int bc_classify_dir(vgl_hip_ctx *c, vgl_hip_graph *g, vgl_bc_cache *k, int d)
{
    hipStream_t st = c->stream;
    const vgl_dir_csr &csr = d == 0 ? g->out : g->in;
    vgl_bc_cache::dir_classes &dc = k->dir[d];
    const int32_t V = g->V;
    VGL_TRY(dc.cls.alloc((size_t)V));
    vgl_dev<int32_t> sizes;
    vgl_dev<unsigned long long> max_row;
    VGL_TRY(sizes.alloc(st, BC_NCLS));
    VGL_TRY(max_row.alloc(st, 1));
    VGL_HIP_TRY(hipMemsetAsync(sizes, 0, sizeof(int32_t) * BC_NCLS, st));
    VGL_HIP_TRY(hipMemsetAsync(max_row, 0, sizeof(unsigned long long), st));
    if (V > 0) {
        hipLaunchKernelGGL(vgl_k_bc_classify, dim3(std::min(bc_grid(V, VGL_BLOCK), 4096u)), dim3(VGL_BLOCK), 0, st, V, csr.rowptr, k->b, dc.cls.p, sizes.p, max_row.p);
        VGL_HIP_TRY(hipGetLastError());
    }
    unsigned long long m = 0;
    VGL_HIP_TRY(hipMemcpyAsync(dc.size, sizes, sizeof(dc.size), hipMemcpyDeviceToHost, st));
    VGL_HIP_TRY(hipMemcpyAsync(&m, max_row, sizeof(m), hipMemcpyDeviceToHost, st));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    dc.max_row = (int64_t)m;
    dc.ready = true;
    return 0;
}

// the classes of the directions a run with `symmetric` reads, under the switches as they stand; *built: something was built now
int bc_ensure(vgl_hip_ctx *c, vgl_hip_graph *g, bool symmetric, vgl_bc_cache **out, bool *built)
{
    int64_t key[4];
    key[0] = vgl_env_int(c, "VGL_BC_SHORT", 32, 0, 1 << 20);
    key[1] = vgl_env_int(c, "VGL_BC_WAVE", 1024, key[0], 1 << 24);
    key[2] = vgl_env_int(c, "VGL_BC_WG", 32768, key[1], 1 << 28);
    key[3] = vgl_rc_env_chunk(c, "VGL_BC_CHUNK");
    *built = false;
    if (!g->bc) g->bc.reset(new vgl_bc_cache());
    vgl_bc_cache *k = g->bc.get();
    if (!std::equal(key, key + 4, k->key)) {
        VGL_HIP_TRY(hipStreamSynchronize(c->stream));           // (kernels of an earlier run may still read the classes)
        k->dir[0].ready = k->dir[1].ready = false;
        k->b = bc_bounds{(int32_t)key[0], (int32_t)key[1], (int32_t)key[2]};
        k->chunk = (int32_t)key[3];
        std::copy(key, key + 4, k->key);
    }
    for (int d = 0; d < (symmetric ? 1 : 2); d++)
        if (!k->dir[d].ready) {
            VGL_TRY(bc_classify_dir(c, g, k, d));
            *built = true;
        }
    *out = k;
    return 0;
}

int bc_validate(const char *who, vgl_hip_ctx *c, vgl_hip_graph *g, int symmetric)
{
    static thread_local std::string msg;
    if (!c || !g) { msg = std::string(who) + ": null argument"; VGL_FAIL(msg.c_str()); }
    if (g->row_begin != 0 || g->row_end != g->V) { msg = std::string(who) + ": graph handle must own all rows (betweenness centrality has no sharded form)"; VGL_FAIL(msg.c_str()); }
    if (!symmetric && !g->in.rowptr) { msg = std::string(who) + ": needs the incoming CSR, or symmetric = 1 from a caller who vouches that the stored graph is symmetric"; VGL_FAIL(msg.c_str()); }
    return 0;
}

// one sweep direction of one run
struct bc_side {
    const vgl_dir_csr *csr;
    const vgl_bc_cache::dir_classes *cls;
    int32_t *order;                     // V
    int32_t *hist, *cursor;             // bucket capacity each
    vgl_rc_chunks ch;                   // hub rows
};

template <bool FWD>
int bc_sweep_level(vgl_hip_ctx *c, const bc_side &s, bc_sweep a, const int64_t *start /* BC_NCLS + 1 offsets into the order */)
{
    static const char *const names[2][BC_NCLS] = {{"bc_backward_short", "bc_backward_wave", "bc_backward_wg", "bc_backward_hub"},
                                                  {"bc_forward_short", "bc_forward_wave", "bc_forward_wg", "bc_forward_hub"}};
    a.rowptr = s.csr->rowptr; a.adj = s.csr->adj;
    a.ch = s.ch;
    for (int k = 0; k < BC_NCLS; k++) {
        const int64_t n = start[k + 1] - start[k];
        if (n <= 0) continue;
        a.order = s.order + start[k];
        a.n = (int32_t)n;
        vgl_timed_launch tl(c, names[FWD ? 1 : 0][k]);
        if (k == BC_SHORT) hipLaunchKernelGGL(vgl_k_bc_short<FWD>, dim3(bc_grid(n * BC_G, VGL_BLOCK)), dim3(VGL_BLOCK), 0, c->stream, a);
        else if (k == BC_WAVE) hipLaunchKernelGGL(vgl_k_bc_wave<FWD>, dim3(bc_grid(n, VGL_WAVES)), dim3(VGL_BLOCK), 0, c->stream, a);
        else if (k == BC_WG) hipLaunchKernelGGL(vgl_k_bc_wg<FWD>, dim3((unsigned)n), dim3(VGL_BLOCK), 0, c->stream, a);
        else {
            hipLaunchKernelGGL(vgl_k_bc_hub, dim3((unsigned)n, (unsigned)s.ch.nchunks), dim3(VGL_BLOCK), 0, c->stream, a);
            hipLaunchKernelGGL(vgl_k_bc_hub_fold<FWD>, dim3(bc_grid(n, VGL_BLOCK)), dim3(VGL_BLOCK), 0, c->stream, a);
        }
    }
    VGL_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int vgl_hip_bc_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int symmetric)
{
    VGL_TRY(bc_validate("bc_prepare", c, g, symmetric));
    vgl_bc_cache *k = nullptr;
    bool built = false;
    VGL_TRY(bc_ensure(c, g, symmetric != 0, &k, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_bc_run(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *sources, int32_t count, int symmetric, int accumulate, double *d_bc, int32_t *d_levels,
                   double *d_sigma, double *d_delta, vgl_hip_bc_stats *stats)
{
    // every refusal comes before the first write to d_bc
    VGL_TRY(bc_validate("bc_run", c, g, symmetric));
    if (count < 0) VGL_FAIL("bc_run: count must not be negative");
    if (!d_bc) VGL_FAIL("bc_run: d_bc must not be NULL");
    if (count > 0 && !sources) VGL_FAIL("bc_run: sources must not be NULL");
    const int32_t V = g->V;
    for (int32_t i = 0; i < count; i++)
        if (sources[i] < 0 || sources[i] >= V) VGL_FAIL("bc_run: source vertex out of range");
    vgl_bc_cache *k = nullptr;
    bool built = false;
    VGL_TRY(bc_ensure(c, g, symmetric != 0, &k, &built));
    hipStream_t st = c->stream;
    vgl_hip_bc_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    if (!accumulate && V > 0) VGL_HIP_TRY(hipMemsetAsync(d_bc, 0, sizeof(double) * (size_t)V, st));
    if (count == 0 || V == 0) {
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (stats) *stats = out;
        return 0;
    }

    // scratch of the call: sigma, coef, levels (unless the caller's are used), one order per direction, the counters, the hub chunk sums
    const int ndir = symmetric ? 1 : 2;
    const int mode = g->in.rowptr ? VGL_HIP_BFS_DIRECTION_OPT : VGL_HIP_BFS_TOP_DOWN;      // (the levels are the same)
    vgl_dev<double> sigma_own, coef, partial;
    vgl_dev<int32_t> levels_own, order[2], buckets, inexact;
    vgl_dev<int64_t> cnt;
    VGL_TRY(sigma_own.alloc(st, (size_t)V));
    VGL_TRY(coef.alloc(st, (size_t)V));
    if (!d_levels) VGL_TRY(levels_own.alloc(st, (size_t)V));
    int32_t *levels = d_levels ? d_levels : levels_own.p;
    for (int d = 0; d < ndir; d++) VGL_TRY(order[d].alloc(st, (size_t)V));
    VGL_TRY(cnt.alloc(st, BC_NCNT));
    VGL_TRY(inexact.alloc(st, (size_t)count));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int64_t) * BC_NCNT, st));
    VGL_HIP_TRY(hipMemsetAsync(inexact, 0, sizeof(int32_t) * (size_t)count, st));
    // side 0 = backward (outgoing CSR), side 1 = forward (incoming CSR, or side 0 again when symmetric)
    bc_side side[2];
    int64_t partial_need = 0;
    for (int d = 0; d < ndir; d++) {
        side[d].csr = d == 0 ? &g->out : &g->in;
        side[d].cls = &k->dir[d];
        side[d].order = order[d];
        side[d].ch = vgl_rc_chunks::of(k->chunk, side[d].cls->max_row);
        partial_need = std::max(partial_need, (int64_t)side[d].cls->size[BC_HUB] * side[d].ch.nchunks);
    }
    if (ndir == 1) side[1] = side[0];
    VGL_TRY(partial.alloc(st, (size_t)partial_need));
    int64_t bucket_cap = 0;                                          // buckets per side the histogram / cursor block holds
    const int32_t per = (int32_t)(vgl_ceil_div(vgl_ceil_div(V, BC_ORDER_BLOCKS), VGL_BLOCK) * VGL_BLOCK);
    const unsigned order_blocks = bc_grid(V, per);
    std::vector<int32_t> h_hist;
    std::vector<int64_t> start;

    for (int32_t si = 0; si < count; si++) {
        const int32_t s = sources[si];
        const bool last = si == count - 1;
        vgl_hip_bfs_stats bst;
        VGL_TRY(vgl_hip_bfs_run(c, g, s, mode, levels, &bst));
        // ---- order ----
        const int32_t level_cap = std::max<int32_t>(bst.levels, 1) + 1;      // a level beyond it would raise the overflow flag
        const int64_t nb = (int64_t)level_cap * BC_NCLS;
        const bool lds = nb <= BC_LDS_BUCKETS;
        if (nb > bucket_cap) {
            bucket_cap = nb + nb / 2;
            VGL_TRY(buckets.alloc(st, (size_t)(bucket_cap * 2 * ndir)));
        }
        for (int d = 0; d < ndir; d++) {
            side[d].hist = buckets.p + (int64_t)d * 2 * bucket_cap;
            side[d].cursor = side[d].hist + bucket_cap;
        }
        if (ndir == 1) side[1] = side[0];
        VGL_HIP_TRY(hipMemsetAsync(buckets, 0, sizeof(int32_t) * (size_t)(bucket_cap * 2 * ndir), st));
        h_hist.assign((size_t)(nb * ndir), 0);
        for (int d = 0; d < ndir; d++) {
            vgl_timed_launch tl(c, "bc_order");
            if (lds) hipLaunchKernelGGL(vgl_k_bc_count<true>, dim3(order_blocks), dim3(VGL_BLOCK), 0, st, V, per, (const int32_t *)levels, (const uint8_t *)side[d].cls->cls.p, level_cap, side[d].hist, cnt.p);
            else hipLaunchKernelGGL(vgl_k_bc_count<false>, dim3(order_blocks), dim3(VGL_BLOCK), 0, st, V, per, (const int32_t *)levels, (const uint8_t *)side[d].cls->cls.p, level_cap, side[d].hist, cnt.p);
            hipLaunchKernelGGL(vgl_k_bc_scan, dim3(1), dim3(VGL_BLOCK), 0, st, (int32_t)nb, (const int32_t *)side[d].hist, side[d].cursor);
            VGL_HIP_TRY(hipMemcpyAsync(h_hist.data() + (size_t)(nb * d), side[d].hist, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
        }
        VGL_HIP_TRY(hipGetLastError());
        int64_t h_cnt[BC_NCNT];
        VGL_HIP_TRY(hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (h_cnt[BC_C_OVERFLOW] != 0) VGL_FAIL("bc_run: internal error (a level beyond the traversal's level count)");
        // bucket starts per side: start[d][level * BC_NCLS + class], one terminator; D = the deepest level index with a vertex
        start.assign((size_t)((nb + 1) * ndir), 0);
        int32_t D = 0;
        int64_t reached = 0;
        for (int d = 0; d < ndir; d++) {
            int64_t run = 0;
            for (int64_t b = 0; b < nb; b++) {
                start[(size_t)((nb + 1) * d + b)] = run;
                run += h_hist[(size_t)(nb * d + b)];
                if (d == 0 && h_hist[(size_t)b]) D = (int32_t)(b / BC_NCLS);
            }
            start[(size_t)((nb + 1) * d + nb)] = run;
            if (d == 0) reached = run;
        }
        if (reached > V) VGL_FAIL("bc_run: internal error (more bucketed vertices than the graph has)");
        for (int d = 0; d < ndir; d++) {
            const int64_t *rp_fwd = (d == ndir - 1) ? side[1].csr->rowptr : nullptr;      // the forward side is the last one (the only one when symmetric)
            const int64_t *rp_bwd = d == 0 ? side[0].csr->rowptr : nullptr;
            vgl_timed_launch tl(c, "bc_order");
            if (lds) hipLaunchKernelGGL(vgl_k_bc_scatter<true>, dim3(order_blocks), dim3(VGL_BLOCK), 0, st, V, per, (const int32_t *)levels, (const uint8_t *)side[d].cls->cls.p, level_cap, side[d].cursor, side[d].order, rp_fwd, rp_bwd, D + 1, cnt.p);
            else hipLaunchKernelGGL(vgl_k_bc_scatter<false>, dim3(order_blocks), dim3(VGL_BLOCK), 0, st, V, per, (const int32_t *)levels, (const uint8_t *)side[d].cls->cls.p, level_cap, side[d].cursor, side[d].order, rp_fwd, rp_bwd, D + 1, cnt.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        // ---- sweeps ----
        double *sigma = (last && d_sigma) ? d_sigma : sigma_own.p;
        double *delta_out = last ? d_delta : nullptr;
        if (last && d_sigma) VGL_HIP_TRY(hipMemsetAsync(d_sigma, 0, sizeof(double) * (size_t)V, st));
        if (delta_out) VGL_HIP_TRY(hipMemsetAsync(delta_out, 0, sizeof(double) * (size_t)V, st));
        hipLaunchKernelGGL(vgl_k_bc_seed, dim3(1), dim3(1), 0, st, sigma, s);
        bc_sweep a;
        memset(&a, 0, sizeof(a));
        a.levels = levels; a.sigma = sigma; a.coef = coef; a.bc = d_bc; a.delta_out = delta_out; a.source = s; a.inexact = inexact.p + si; a.partial = partial;
        const int64_t *fs = start.data() + (size_t)((nb + 1) * (ndir - 1)), *bs = start.data();
        for (int32_t li = 1; li <= D; li++) {                       // level index li holds the vertices with levels == li + 1
            a.gather = sigma; a.want = li;
            VGL_TRY(bc_sweep_level<true>(c, side[1], a, fs + (int64_t)li * BC_NCLS));
        }
        {
            const int64_t n = bs[(int64_t)(D + 1) * BC_NCLS] - bs[(int64_t)D * BC_NCLS];
            vgl_timed_launch tl(c, "bc_leaf");
            hipLaunchKernelGGL(vgl_k_bc_leaf, dim3(bc_grid(n, VGL_BLOCK)), dim3(VGL_BLOCK), 0, st, (const int32_t *)(side[0].order + bs[(int64_t)D * BC_NCLS]), (int32_t)n, (const double *)sigma, coef.p);
        }
        for (int32_t li = D - 1; li >= 0; li--) {
            a.gather = coef; a.want = li + 2;
            VGL_TRY(bc_sweep_level<false>(c, side[0], a, bs + (int64_t)li * BC_NCLS));
        }
        VGL_HIP_TRY(hipGetLastError());
        out.sources++;
        out.max_depth = std::max(out.max_depth, D);
        out.levels_total += D + 1;
        out.reached_total += reached;
        // the model: the traversal's own bytes; per order pass levels + class read twice and the order written; per sweep
        // 8 bytes per entry walked (adjacency + the endpoint's level) and the per-row reads and writes -- the 8-byte gathers of matching entries are left out
        out.algorithmic_bytes += bst.algorithmic_bytes + (int64_t)ndir * (10 * (int64_t)V + 4 * reached) + 28 * (reached - 1) + 52 * reached;
    }
    std::vector<int32_t> h_inexact((size_t)count);
    int64_t h_cnt[BC_NCNT];
    VGL_HIP_TRY(hipMemcpyAsync(h_inexact.data(), inexact, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, st));
    VGL_HIP_TRY(hipMemcpyAsync(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    for (int32_t v : h_inexact) out.sigma_inexact += v != 0;
    out.edges_forward = h_cnt[BC_C_FWD];
    out.edges_backward = h_cnt[BC_C_BWD];
    out.algorithmic_bytes += 8 * (out.edges_forward + out.edges_backward);
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
