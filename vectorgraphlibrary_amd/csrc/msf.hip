// msf.hip -- minimum spanning forest (Boruvka) of the simple undirected graph underlying the stored outgoing CSR, with float32 weights per stored entry.
// The contract is written out in include/vgl_hip.h; DESIGN section 17 has the round, the kernel resources and the bytes model.
//
// Prepare (once per graph, cached on the handle): the symmetric simple CSR, the edge numbering (eid per slot, endpoints) and slot_eid[s] = the
// undirected edge of the STORED outgoing entry s, -1 for a loop, are simple.hip's (vgl_simple_ensure_slot_ids), shared with kcore and ktruss.
// Structure is per graph, values are per weights.
//
// Fold (per run): wkey[e] = min over the stored entries of e of the order-preserving uint32 image of the weight (-0.0 canonicalised, sign bit
// flipped, negatives complemented): one streaming pass, an integer atomicMin per entry, NaNs counted for the error.
//
// Round (comp[v] = the root vertex of v's component; best[c] = the smallest key  wkey << 32 | eid  of an edge that leaves component c):
//   min-edge  the live rows, one kernel per row class (short: 8 lanes per row, wave, workgroup per chunk): a lane keeps the smallest key over its
//             entries u with comp[u] != comp[v]; one 64-bit atomicMin per row on best[comp[v]], skipped when the slot already holds a smaller key
//             (it only falls within a round); a row WITH a crossing entry is appended to the live list of the next round, a row without one never
//             gets one again (components only grow) and is dropped.
//   hook      every root c with a pick e: d = the component at the far end; if d picked e too and c < d, c stays a root, otherwise parent[c] = d,
//             in_forest[e] = 1 and the edge is counted.  Under the strict order (weight, id) mutual picks are the only cycles.
//   flatten   chase parent (read-only) from every old root to its new root, into a second array; comp[v] = root[comp[v]]; best reset for the roots.
//   publish   list tails, picks and entries walked into the pinned mirror: one host read per round.  The loop ends on a round with no pick.
// The live lists are one ring per class of twice the class's rows: a round reads [head, tail) and appends behind tail, positions taken modulo the
// capacity; appends are staged per wave in LDS and cost one returning atomic per 64 or more rows.  No cooperative launch, no grid barrier.
#include "vgl_simple.h"
#include "vgl_rowclass.h"
#include "vgl_prim.h"
#include <cstring>
#include <algorithm>
#include <climits>

namespace {

constexpr int64_t MSF_MAX_GRID = 2048;            // workgroups of a grid-stride kernel
constexpr int MSF_MAX_ROUNDS = 64;                // (a run has at most ceil(log2 V) <= 31 rounds that add an edge, plus the empty one)
constexpr int MSF_SUM_GRID = 1024;                // partials of the weight sum at most
constexpr unsigned long long MSF_NONE = ~0ull;    // "no crossing edge" in best (a byte pattern: one memset arms the array)
enum {
    MSF_TAIL = 0,       // + class: rows appended to the class ring so far (cumulative)
    MSF_PICKS = 3,      // edges the hooks added to the forest so far
    MSF_WALK = 4,       // adjacency entries the min-edge passes walked so far
    MSF_NAN = 5,        // NaN weights on non-loop entries
    MSF_ROWS = 6,       // + class: rows with an entry, per class
    MSF_NCNT = 9
};
static_assert(MSF_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

struct msf_graph {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    const int32_t *eid;          // edge id of every adjacency slot
    const uint32_t *wkey;        // folded weight of every edge, as an order-preserving uint32
    const int32_t *comp;
    unsigned long long *best;
};

// float -> uint32 that orders as the numbers do (-0.0 == +0.0; -inf smallest, +inf largest), and back
__device__ __forceinline__ uint32_t msf_key_of(float w)
{
    uint32_t b = __float_as_uint(w);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float msf_weight_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// ---- fold ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_fold(int64_t E, const int32_t *slot_eid, const float *w, uint32_t *wkey, unsigned long long *cnt)
{
    int64_t nans = 0;
    for (int64_t s = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; s < E; s += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t e = slot_eid[s];
        if (e < 0) continue;
        const float x = w[s];
        if (x != x) { nans++; continue; }
        atomicMin(wkey + e, msf_key_of(x));
    }
    vgl_wave_flush_add(cnt + MSF_NAN, nans);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_edge_weight(int32_t ne, const uint32_t *wkey, float *out)
{
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < ne; e += (int64_t)gridDim.x * VGL_BLOCK) out[e] = msf_weight_of(wkey[e]);
}

// ---- the live lists ----
// (appends: vgl_rc_stage onto the ring of the class, one returning atomic per 64 or more rows)
// the rows with an entry, by their length; the filling pass (comp != nullptr) also sets comp[v] = v for every vertex
struct msf_row_src {
    const int32_t *deg; vgl_rc_bounds b; int32_t *comp;
    __device__ __forceinline__ int cls(int64_t v, int64_t &) const
    {
        if (comp) comp[v] = (int32_t)v;
        const int32_t d = deg[v];
        return d > 0 ? vgl_rc_class_of(d, b) : -1;
    }
};

// ---- the min-edge pass ----
// the smallest key over the entries lo, lo + stride, ... < hi whose far end lies in another component than cv
__device__ __forceinline__ unsigned long long msf_walk(int64_t lo, int64_t hi, int stride, int32_t cv, const msf_graph &g)
{
    unsigned long long m = MSF_NONE;
    for (int64_t i = lo; i < hi; i += stride)
        if (g.comp[g.adj[i]] != cv) {
            const int32_t e = g.eid[i];
            m = min(m, (unsigned long long)g.wkey[e] << 32 | (unsigned long long)(uint32_t)e);
        }
    return m;
}
// best[c] = min(best[c], key).  The slot only falls within a round, so a stored key that is already smaller settles it without the atomic.
__device__ __forceinline__ void msf_offer(unsigned long long *slot, unsigned long long key)
{
    if (vgl_load_agent(slot) > key) atomicMin(slot, key);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_min_short(msf_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, unsigned long long *cnt)
{
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    const int gi = threadIdx.x & (VGL_RC_G - 1), lane = vgl_lane();
    int64_t walked = 0;
    for (int64_t base = (int64_t)blockIdx.x * (VGL_BLOCK / VGL_RC_G); base < n; base += (int64_t)gridDim.x * (VGL_BLOCK / VGL_RC_G)) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x / VGL_RC_G;
        int32_t v = 0, cv = 0;
        int64_t lo = 0, hi = 0;
        if (i < n) {
            v = R.rows[(head + (unsigned long long)i) % R.cap];
            cv = g.comp[v];
            lo = g.rowptr[v]; hi = g.rowptr[v + 1];
        }
        unsigned long long m = msf_walk(lo + gi, hi, VGL_RC_G, cv, g);
#pragma unroll
        for (int o = VGL_RC_G / 2; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        if (gi == 0) walked += hi - lo;
        const bool found = gi == 0 && m != MSF_NONE;
        // the rows of this wave that share the first found row's component go to its slot as one
        const unsigned long long f = __ballot(found);
        if (f) {                                                      // (uniform)
            const int leader = __ffsll((long long)f) - 1;
            const int32_t c0 = __shfl(cv, leader);
            const bool same = found && cv == c0;
            const unsigned long long k0 = vgl_rc_team<VGL_RC_WAVE>::min_of(same ? m : MSF_NONE);
            if (lane == leader) msf_offer(g.best + c0, k0);
            else if (found && !same) msf_offer(g.best + cv, m);
        }
        st[0].keep(found, v, R, cnt + MSF_TAIL + VGL_RC_SHORT);
    }
    st[0].flush(R, cnt + MSF_TAIL + VGL_RC_SHORT);
    vgl_wave_flush_add(cnt + MSF_WALK, walked);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_min_wave(msf_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, unsigned long long *cnt)
{
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    const int lane = vgl_lane();
    int64_t walked = 0;
    for (int64_t i = (int64_t)blockIdx.x * VGL_WAVES + vgl_wave(); i < n; i += (int64_t)gridDim.x * VGL_WAVES) {      // (uniform over the wave)
        const int32_t v = R.rows[(head + (unsigned long long)i) % R.cap];
        const int32_t cv = g.comp[v];
        const int64_t lo = g.rowptr[v], hi = g.rowptr[v + 1];
        const unsigned long long m = vgl_rc_team<VGL_RC_WAVE>::min_of(msf_walk(lo + lane, hi, 64, cv, g));
        const bool found = lane == 0 && m != MSF_NONE;
        if (lane == 0) walked += hi - lo;
        if (found) msf_offer(g.best + cv, m);
        st[0].keep(found, v, R, cnt + MSF_TAIL + VGL_RC_WAVE);
    }
    st[0].flush(R, cnt + MSF_TAIL + VGL_RC_WAVE);
    vgl_wave_flush_add(cnt + MSF_WALK, walked);
}
// work item w = (row i of the segment, piece k of its chunks): an item past the end of its row has nothing to do.
// A row is appended by the first of its chunks that finds a crossing entry: stamp[position in the segment] = the round.
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_min_wg(msf_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, vgl_rc_chunks ch, int32_t round, int32_t *stamp,
                                                               unsigned long long *cnt)
{
    __shared__ unsigned long long s_red[VGL_WAVES];
    const int64_t total = (int64_t)n * ch.nchunks;
    int64_t walked = 0;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {         // (uniform over the workgroup)
        int64_t i, k, lo, hi;
        ch.split(w, &i, &k);
        const int32_t v = R.rows[(head + (unsigned long long)i) % R.cap];
        if (!ch.range(g.rowptr[v], g.rowptr[v + 1], k, &lo, &hi)) continue;
        const int32_t cv = g.comp[v];
        unsigned long long m = vgl_rc_team<VGL_RC_WAVE>::min_of(msf_walk(lo + threadIdx.x, hi, VGL_BLOCK, cv, g));
        __syncthreads();
        if (vgl_lane() == 0) s_red[vgl_wave()] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < VGL_WAVES; k++) m = min(m, s_red[k]);
            walked += hi - lo;
            if (m != MSF_NONE) {
                msf_offer(g.best + cv, m);
                if (atomicExch(stamp + i, round) != round) {
                    const unsigned long long pos = atomicAdd(cnt + MSF_TAIL + VGL_RC_WG, 1ull);
                    R.rows[pos % R.cap] = v;
                }
            }
        }
    }
    if (threadIdx.x == 0 && walked) atomicAdd(cnt + MSF_WALK, (unsigned long long)walked);
}

// ---- hook, flatten ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_hook(int32_t V, const int32_t *comp, const unsigned long long *best, const int32_t *eu, const int32_t *ev, int32_t *parent,
                                                             uint8_t *in_forest, unsigned long long *cnt)
{
    int64_t picks = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        if (comp[v] != (int32_t)v) continue;                          // roots only
        const unsigned long long k = best[v];
        int32_t p = (int32_t)v;
        if (k != MSF_NONE) {
            const int32_t e = (int32_t)(uint32_t)k;
            const int32_t ca = comp[eu[e]], cb = comp[ev[e]];
            const int32_t d = ca == (int32_t)v ? cb : ca;
            if (!(best[d] == k && (int32_t)v < d)) {                  // not the lower side of a mutual pick: v hooks, and counts the edge
                p = d;
                in_forest[e] = 1;
                picks++;
            }
        }
        parent[v] = p;
    }
    vgl_wave_flush_add(cnt + MSF_PICKS, picks);
}
// root[c] = the root of old root c under parent (read-only here; acyclic, and the walk is bounded by V all the same)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_chase(int32_t V, const int32_t *comp, const int32_t *parent, int32_t *root)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        if (comp[v] != (int32_t)v) continue;
        int32_t x = (int32_t)v;
        for (int32_t it = 0; it < V; it++) {
            const int32_t p = parent[x];
            if (p == x) break;
            x = p;
        }
        root[v] = x;
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_relabel(int32_t V, int32_t *comp, const int32_t *root, unsigned long long *best)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t c = root[comp[v]];
        comp[v] = c;
        if (c == (int32_t)v) best[v] = MSF_NONE;
    }
}
// ---- after the loop ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_min_id(int32_t V, const int32_t *comp, int32_t *minid)      // minid[c] starts as c
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t c = comp[v];
        if ((int32_t)v < c) atomicMin(minid + c, (int32_t)v);
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_component(int32_t V, const int32_t *comp, const int32_t *minid, int32_t *out)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) out[v] = minid[comp[v]];
}
// The float64 sum of the forest edges' weights, in a shape fixed by E' alone: thread t of workgroup b adds the edges b * 256 + t + k * grid * 256 in
// ascending k, the wave adds by the xor tree, thread 0 the four waves in order; then one workgroup does the same over the partials.
__device__ __forceinline__ double msf_block_sum(double x, double *s_red)
{
    x = vgl_wave_reduce_add(x);
    __syncthreads();
    if (vgl_lane() == 0) s_red[vgl_wave()] = x;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < VGL_WAVES; k++) t += s_red[k];
    return t;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_sum_partials(int32_t ne, const uint8_t *in_forest, const uint32_t *wkey, double *partials)
{
    __shared__ double s_red[VGL_WAVES];
    double x = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < ne; e += (int64_t)gridDim.x * VGL_BLOCK)
        if (in_forest[e]) x += (double)msf_weight_of(wkey[e]);
    x = msf_block_sum(x, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = x;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msf_sum_final(int32_t n, const double *partials, double *out)
{
    __shared__ double s_red[VGL_WAVES];
    double x = 0.0;
    for (int i = threadIdx.x; i < n; i += VGL_BLOCK) x += partials[i];
    x = msf_block_sum(x, s_red);
    if (threadIdx.x == 0) *out = x;
}

int msf_check_handle(vgl_hip_graph *g, const char *msg)
{
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL(msg);
    return 0;
}

}  // namespace

extern "C" {

int vgl_hip_msf_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int64_t *undirected_edges)
{
    if (!c || !g) VGL_FAIL("msf_prepare: null argument");
    VGL_TRY(msf_check_handle(g, "msf_prepare: graph handle must own all rows (the minimum spanning forest has no sharded form)"));
    const vgl_simple_cache *sg = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_slot_ids(c, g, &sg, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    if (undirected_edges) *undirected_edges = sg->ne;
    return 0;
}

int vgl_hip_msf_run(vgl_hip_ctx *c, vgl_hip_graph *g, const float *d_weights, int32_t *d_edge_u, int32_t *d_edge_v, float *d_edge_weight, uint8_t *d_in_forest,
                    int32_t *d_component, vgl_hip_msf_stats *stats)
{
    if (!c || !g) VGL_FAIL("msf_run: null argument");
    VGL_TRY(msf_check_handle(g, "msf_run: graph handle must own all rows (the minimum spanning forest has no sharded form)"));
    if (!d_in_forest) VGL_FAIL("msf_run: d_in_forest must not be NULL");
    if (!d_weights && g->out.edges > 0) VGL_FAIL("msf_run: d_weights must not be NULL (one float32 per stored outgoing entry)");
    if ((d_edge_u == nullptr) != (d_edge_v == nullptr)) VGL_FAIL("msf_run: d_edge_u and d_edge_v go together (both or neither)");
    const vgl_simple_cache *sg = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_slot_ids(c, g, &sg, &built));
    const int32_t V = g->V;
    const int64_t E = g->out.edges;
    hipStream_t st = c->stream;
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_MSF_SHORT", "VGL_MSF_WAVE");
    const int64_t chunk_env = vgl_rc_env_chunk(c, "VGL_MSF_CHUNK");
    vgl_hip_msf_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    out.undirected_edges = sg->ne;
    out.components = V;
    const int32_t ne = (int32_t)sg->ne;

    // the one host-visible read of a step: the counters through the pinned mirror
    vgl_dev<unsigned long long> cnt;
    VGL_TRY(cnt.alloc(st, MSF_NCNT));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * MSF_NCNT, st));
    auto read = [&]() -> int {
        return vgl_publish_counters(c, "msf_publish", cnt, MSF_NCNT);
    };

    // ---- fold; the NaN check comes before any output is written ----
    vgl_dev<uint32_t> wkey;
    VGL_TRY(wkey.alloc(st, (size_t)ne));
    if (ne > 0) {
        VGL_HIP_TRY(hipMemsetAsync(wkey, 0xFF, sizeof(uint32_t) * (size_t)ne, st));
        {
            vgl_timed_launch tl(c, "msf_fold");
            hipLaunchKernelGGL(vgl_k_msf_fold, dim3(vgl_grid(E, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, E, (const int32_t *)sg->slot_eid.p, d_weights, wkey.p, cnt.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(read());
        if (c->h_counters[MSF_NAN] != 0) VGL_FAIL("msf_run: weights holds a NaN on an entry that is not a loop (the order of the edges needs numbers)");
    }

    if (V > 0 && ne == 0 && d_component) {
        hipLaunchKernelGGL(vgl_k_iota, dim3(vgl_grid(V, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, d_component);
        VGL_HIP_TRY(hipGetLastError());
    }
    if (ne == 0) {
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (stats) *stats = out;
        return 0;
    }
    if (d_edge_u) {
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_u, sg->eu, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_v, sg->ev, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
    }
    if (d_edge_weight) {
        hipLaunchKernelGGL(vgl_k_msf_edge_weight, dim3(vgl_grid(ne, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, ne, (const uint32_t *)wkey.p, d_edge_weight);
        VGL_HIP_TRY(hipGetLastError());
    }
    VGL_HIP_TRY(hipMemsetAsync(d_in_forest, 0, (size_t)ne, st));

    // ---- scratch of the call, all of it drawn before the loop ----
    vgl_dev<int32_t> comp, parent, root, stamp;
    vgl_dev<unsigned long long> best;
    vgl_dev<double> partials;
    const int sum_grid = (int)vgl_grid(ne, VGL_BLOCK, MSF_SUM_GRID);
    VGL_TRY(comp.alloc(st, (size_t)V));
    VGL_TRY(parent.alloc(st, (size_t)V));
    VGL_TRY(root.alloc(st, (size_t)V));
    VGL_TRY(best.alloc(st, (size_t)V));
    VGL_TRY(partials.alloc(st, (size_t)sum_grid + 1));
    VGL_HIP_TRY(hipMemsetAsync(best, 0xFF, sizeof(unsigned long long) * (size_t)V, st));      // MSF_NONE
    vgl_rc_lists<vgl_rc_ring> L;                 // one ring per class, of twice the class's rows
    msf_row_src src{sg->csr.deg, b, nullptr};
    VGL_TRY(L.count(c, nullptr, "msf_publish", src, V, MSF_MAX_GRID, cnt.p, MSF_NCNT, MSF_ROWS, -1, -1, -1, nullptr,
                    "msf_run: internal error (the classes do not add up to the rows that have an entry)"));
    const int64_t *rows = L.rows, rows_total = rows[0] + rows[1] + rows[2];
    for (int k = 0; k < VGL_RC_N; k++)
        if (rows[k] > V) VGL_FAIL("msf_run: internal error (more rows in a class than vertices)");
    if (rows_total < 2 || rows_total > V) VGL_FAIL("msf_run: internal error (the classes do not add up to the rows that have an entry)");
    VGL_TRY(stamp.alloc(st, (size_t)rows[VGL_RC_WG]));
    VGL_HIP_TRY(hipMemsetAsync(stamp, 0, sizeof(int32_t) * (size_t)std::max<int64_t>(rows[VGL_RC_WG], 1), st));
    src.comp = comp.p;
    VGL_TRY(L.fill(c, nullptr, src, V, MSF_MAX_GRID, 2, nullptr, cnt + MSF_TAIL));
    const vgl_rc_ring *R = L.l;

    msf_graph mg;
    mg.rowptr = sg->csr.rowptr; mg.adj = sg->csr.adj; mg.eid = sg->eid; mg.wkey = wkey; mg.comp = comp; mg.best = best;
    const vgl_rc_chunks ch = vgl_rc_chunks::of(chunk_env, sg->csr.max_deg);
    vgl_rc_window w;                             // the live rows: [head, tail) of the rings, cumulative positions
    for (int k = 0; k < VGL_RC_N; k++) w.tail[k] = rows[k];
    const char *const slot[VGL_RC_N] = {"msf_min_short", "msf_min_wave", "msf_min_wg"};
    int64_t picks = 0;
    int32_t rounds = 0;
    for (int32_t round = 1;; round++) {
        if (round > MSF_MAX_ROUNDS) VGL_FAIL("msf_run: internal error (more rounds than a forest can take)");
        // ---- the min-edge pass: a launch per class that has live rows ----
        VGL_TRY(vgl_rc_launch(c, slot, w, [&](int cls, int64_t n) {
            const unsigned long long head = (unsigned long long)w.head[cls];
            if (cls == VGL_RC_SHORT)
                hipLaunchKernelGGL(vgl_k_msf_min_short, dim3(vgl_grid(n * VGL_RC_G, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, R[cls], head, (int32_t)n, cnt.p);
            else if (cls == VGL_RC_WAVE)
                hipLaunchKernelGGL(vgl_k_msf_min_wave, dim3(vgl_grid(n, VGL_WAVES, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, R[cls], head, (int32_t)n, cnt.p);
            else
                hipLaunchKernelGGL(vgl_k_msf_min_wg, dim3(vgl_grid(n * ch.nchunks, 1, 4 * MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, R[cls], head, (int32_t)n, ch, round, stamp.p,
                                   cnt.p);
        }));
        {
            vgl_timed_launch tl(c, "msf_hook");
            hipLaunchKernelGGL(vgl_k_msf_hook, dim3(vgl_grid(V, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)comp.p, (const unsigned long long *)best.p, sg->eu, sg->ev, parent.p,
                               d_in_forest, cnt.p);
        }
        {
            vgl_timed_launch tl(c, "msf_flatten");
            hipLaunchKernelGGL(vgl_k_msf_chase, dim3(vgl_grid(V, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)comp.p, (const int32_t *)parent.p, root.p);
        }
        {
            vgl_timed_launch tl(c, "msf_flatten");
            hipLaunchKernelGGL(vgl_k_msf_relabel, dim3(vgl_grid(V, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, comp.p, (const int32_t *)root.p, best.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(read());
        const int64_t was[VGL_RC_N] = {w.n(0), w.n(1), w.n(2)};
        VGL_TRY(w.advance(c->h_counters + MSF_TAIL, INT64_MAX, "msf_run: internal error (a live list grew)"));      // (a ring: positions have no end)
        for (int k = 0; k < VGL_RC_N; k++)
            if (w.n(k) > was[k]) VGL_FAIL("msf_run: internal error (a live list grew)");
        const int64_t now = c->h_counters[MSF_PICKS];
        if (now < picks || now >= V) VGL_FAIL("msf_run: internal error (more forest edges than a forest has)");
        if (now == picks) break;                                      // a round with no pick: every live row saw its own component only
        picks = now;
        rounds++;
        if (w.live() == 0) break;                                         // no row has a crossing entry left
    }

    // ---- the smallest vertex id of every component; the weight of the forest ----
    if (d_component) {
        hipLaunchKernelGGL(vgl_k_iota, dim3(vgl_grid(V, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, root.p);
        hipLaunchKernelGGL(vgl_k_msf_min_id, dim3(vgl_grid(V, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)comp.p, root.p);
        hipLaunchKernelGGL(vgl_k_msf_component, dim3(vgl_grid(V, VGL_BLOCK, MSF_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)comp.p, (const int32_t *)root.p, d_component);
        VGL_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(vgl_k_msf_sum_partials, dim3(sum_grid), dim3(VGL_BLOCK), 0, st, ne, (const uint8_t *)d_in_forest, (const uint32_t *)wkey.p, partials.p);
    hipLaunchKernelGGL(vgl_k_msf_sum_final, dim3(1), dim3(VGL_BLOCK), 0, st, sum_grid, (const double *)partials.p, partials.p + sum_grid);
    VGL_HIP_TRY(hipGetLastError());
    double total = 0.0;
    VGL_HIP_TRY(hipMemcpyAsync(&total, partials.p + sum_grid, sizeof(double), hipMemcpyDeviceToHost, st));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.rounds = rounds;
    out.forest_edges = picks;
    out.components = V - picks;
    out.entries_walked = c->h_counters[MSF_WALK];
    out.algorithmic_bytes = 8 * E + 5 * (int64_t)ne + 12 * out.entries_walked + 20 * (int64_t)V * rounds;
    out.total_weight = total;
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
