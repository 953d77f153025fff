// ktruss.hip -- k-truss decomposition (truss number and initial triangle support of every edge) of the simple undirected graph underlying the stored
// outgoing CSR.  The contract is written out in include/vgl_hip.h; DESIGN section 16 has the rule, the kernel resources and the bytes model.
//
// Prepare (once per graph, cached on the handle): the symmetric simple CSR, rows ascending by id, and the numbering of its edges (eid of every slot,
// lo / hi of every edge, ids ascending with (lo, hi)) are simple.hip's (vgl_simple_ensure_edge_ids), shared with kcore and msf.
//
// Support (per run; one pass, every support written once, no atomics on them): the edges are appended to one list per class of the SHORTER row's
// length (<= VGL_KTRUSS_SHORT: 8 lanes per edge, <= VGL_KTRUSS_WAVE: a wavefront, longer: a workgroup); the lanes stride over the shorter row and
// binary-search the longer.  The sums (supports, entries walked) and the largest support cost one atomic each per wave of a bounded grid.
//
// Peel (level-synchronous; sup = the working supports; stamp[e] = the sub-round sequence number at which e entered a frontier, 0 = never):
//   k change   k = min over the alive edges (stamp 0) of sup, + 2 (a device reduction); the alive edges with sup <= k - 2 are the first frontier of k.
//   sub-round  number s: an expanded edge e1 = (u, v) has truss k (written when it was appended); for every common neighbour w, e2 = (a, w) and
//              e3 = (b, w) from eid at the two matched slots:  one of them stamped below s: the triangle went earlier;  neither stamped s: both are
//              decremented;  exactly one stamped s (say e2): e3 is decremented iff e1 < e2;  both: nothing.  Every triangle that is whole at the
//              start of the sub-round and has an edge in the frontier is so destroyed exactly once.
//   decrement  old = atomicSub(&sup[e], 1);  old == k - 1: this thread appends e (stamp s + 1, truss k);  old <= k - 2: put back.  While sup is above
//              k - 2 it only falls; at or below, every decrement that lands is put back: the crossing happens in one thread (kcore's argument).
// An edge enters a frontier exactly once, so the frontiers are consecutive segments of one list per class; appends are aggregated per wave (ballot +
// one returning atomic).  The host reads the pinned mirror once per sub-round.  No cooperative launch, no grid barrier, no workgroup waits for another:
// every turn of the host loop expands a non-empty frontier or changes k.
#include "vgl_simple.h"
#include "vgl_rowclass.h"
#include <cstring>
#include <algorithm>
#include <climits>

namespace {

constexpr int64_t KT_MAX_GRID = 8192;           // workgroups of a grid-stride kernel: bounds the per-wave atomics on the shared counters
constexpr int64_t KT_NO_K = 0x7F7F7F7F7F7F7F7Fll;      // "no alive edge" in KT_K (a byte pattern: one memset arms the min kernel)
enum {
    KT_TAIL = 0,        // + class: entries appended to the class list so far
    KT_M = 3,           // shorter-row lengths of the appended edges, summed = entries the peel walks once they are all expanded
    KT_K = 4,           // the min kernel's result: the smallest support of an alive edge
    KT_SUM = 5,         // sum of the initial supports = 3 * triangles
    KT_WALK = 6,        // entries the support pass walked
    KT_MAXSUP = 7,      // the largest initial support
    KT_NCNT = 8
};
static_assert(KT_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

struct kt_lists { int32_t *list[VGL_RC_N]; int32_t cap; };      // one list of edge ids per class, `cap` entries each
struct kt_graph {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    const int32_t *deg;
    const int32_t *eid;          // edge id of every adjacency slot
    const int32_t *eu, *ev;      // lo, hi of every edge
    int32_t *sup;                // working supports
    int32_t *stamp;              // sub-round at which the edge entered a frontier; 0: never
    int32_t *truss;
    vgl_rc_bounds b;             // classes of the shorter row's length
    kt_lists L;
};
__device__ __forceinline__ int32_t kt_shorter(int32_t e, const kt_graph &g) { return min(g.deg[g.eu[e]], g.deg[g.ev[e]]); }

// ---- shared device pieces ----
// (appends: vgl_wave_append, one returning atomic per wave and class)
// the two rows of an edge: [a_lo, a_hi) is walked (the shorter; ties: the lower endpoint's), [b_lo, b_hi) is searched
struct kt_rows { int64_t a_lo, a_hi, b_lo, b_hi; };
__device__ __forceinline__ kt_rows kt_rows_of(int32_t e, const kt_graph &g)
{
    const int32_t u = g.eu[e], v = g.ev[e];
    const int64_t u0 = g.rowptr[u], u1 = g.rowptr[u + 1], v0 = g.rowptr[v], v1 = g.rowptr[v + 1];
    return (u1 - u0 <= v1 - v0) ? kt_rows{u0, u1, v0, v1} : kt_rows{v0, v1, u0, u1};
}

// ---- support ----
// the triangles of one edge that this lane sees: lane `li` of `stride` strides over the walked row
__device__ __forceinline__ int32_t kt_count(const kt_rows &r, int li, int stride, const int32_t *adj)
{
    int32_t n = 0;
    for (int64_t i = r.a_lo + li; i < r.a_hi; i += stride)
        if (vgl_slot_of(adj, r.b_lo, r.b_hi, adj[i]) >= 0) n++;
    return n;
}
__device__ __forceinline__ void kt_support_done(unsigned long long *cnt, int64_t sum, int64_t walk, int32_t mx)
{
    vgl_wave_flush_add(cnt + KT_SUM, sum);
    vgl_wave_flush_add(cnt + KT_WALK, walk);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    if (vgl_lane() == 0 && mx) atomicMax(cnt + KT_MAXSUP, (unsigned long long)mx);
}
// all edges into the class lists (the lists are the peel's: the support pass borrows them, the tails are reset before the peel)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ktruss_classify(int32_t ne, kt_graph g, unsigned long long *cnt)
{
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < ne; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t e = base + threadIdx.x;
        const bool want = e < ne;
        vgl_wave_append<VGL_RC_N>(want, (int32_t)e, want ? vgl_rc_class_of(kt_shorter((int32_t)e, g), g.b) : 0, g.L.list, g.L.cap, cnt + KT_TAIL);
    }
}
// a team per edge: its triangles
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ktruss_sup(const int32_t *edges, int32_t n, kt_graph g, unsigned long long *cnt)
{
    using T = vgl_rc_team<CLS>;
    int64_t sum = 0, walk = 0;
    int32_t mx = 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        const int32_t e = has ? edges[i] : 0;
        kt_rows r{0, 0, 0, 0};
        if (has) r = kt_rows_of(e, g);
        const int32_t t = T::sum_of(kt_count(r, T::lane(), T::LANES, g.adj));
        if (T::lead() && has) { g.sup[e] = t; sum += t; walk += r.a_hi - r.a_lo; mx = max(mx, t); }
    }
    kt_support_done(cnt, sum, walk, mx);
}

// ---- the peel ----
// One candidate decrement of edge e at level k in sub-round s (active = this lane holds one).  Every lane of the wave calls.
__device__ __forceinline__ void kt_dec(bool active, int32_t e, int32_t k, int32_t s, const kt_graph &g, unsigned long long *tail, int64_t &m_acc)
{
    bool want = false;
    int cls = 0;
    if (active && vgl_load_agent(g.sup + e) > k - 2) {                // (a stale value can only be too large: that costs an atomic)
        const int32_t old = atomicSub(g.sup + e, 1);
        if (old == k - 1) {
            const int32_t len = kt_shorter(e, g);
            vgl_store_agent(g.stamp + e, s + 1);
            g.truss[e] = k;
            want = true;
            cls = vgl_rc_class_of(len, g.b);
            m_acc += len;
        } else if (old <= k - 2) atomicAdd(g.sup + e, 1);
    }
    vgl_wave_append<VGL_RC_N>(want, e, cls, g.L.list, g.L.cap, tail);
}
// The frontier edge e1 with rows r, lane `li` of `stride`.  Uniform over the wave as long as every lane of the wave calls (has = this lane has an edge).
__device__ __forceinline__ void kt_expand(bool has, int32_t e1, const kt_rows &r, int li, int stride, int32_t k, int32_t s, const kt_graph &g,
                                          unsigned long long *tail, int64_t &m_acc)
{
    int64_t i = has ? r.a_lo + li : 0;
    const int64_t end = has ? r.a_hi : 0;
    while (__any(i < end)) {
        bool dec2 = false, dec3 = false;
        int32_t e2 = 0, e3 = 0;
        if (i < end) {
            const int64_t j = vgl_slot_of(g.adj, r.b_lo, r.b_hi, g.adj[i]);
            if (j >= 0) {
                e2 = g.eid[i]; e3 = g.eid[j];
                const int32_t s2 = vgl_load_agent(g.stamp + e2), s3 = vgl_load_agent(g.stamp + e3);
                const bool gone = (s2 != 0 && s2 < s) || (s3 != 0 && s3 < s);       // removed in an earlier sub-round or level
                const bool in2 = s2 == s, in3 = s3 == s;                            // (a stamp s + 1 was set in this sub-round: still alive in it)
                if (!gone) {
                    dec2 = !in2 && (!in3 || e1 < e3);
                    dec3 = !in3 && (!in2 || e1 < e2);
                }
            }
        }
        kt_dec(dec2, e2, k, s, g, tail, m_acc);
        kt_dec(dec3, e3, k, s, g, tail, m_acc);
        i += stride;
    }
}
// cnt[KT_K] = min(sup) over the alive edges
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ktruss_min(int32_t ne, const int32_t *sup, const int32_t *stamp, unsigned long long *cnt)
{
    int m = INT_MAX;
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < ne; e += (int64_t)gridDim.x * VGL_BLOCK)
        if (stamp[e] == 0) m = min(m, sup[e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
    if (vgl_lane() == 0 && m != INT_MAX) atomicMin(cnt + KT_K, (unsigned long long)m);
}
// the first frontier of k = cnt[KT_K] + 2, sub-round s_next: the alive edges with sup <= k - 2 (nothing when no edge is alive or k has reached k_limit)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ktruss_scan(int32_t ne, kt_graph g, int32_t s_next, int32_t k_limit, unsigned long long *cnt)
{
    const unsigned long long m64 = cnt[KT_K];
    if (m64 == (unsigned long long)KT_NO_K || (k_limit > 0 && m64 + 2 >= (unsigned long long)k_limit)) return;
    const int32_t k = (int32_t)m64 + 2;
    int64_t m_acc = 0;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < ne; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t e = base + threadIdx.x;
        bool want = false;
        int cls = 0;
        if (e < ne && g.stamp[e] == 0 && g.sup[e] <= k - 2) {
            const int32_t len = kt_shorter((int32_t)e, g);
            g.stamp[e] = s_next;
            g.truss[e] = k;
            want = true;
            cls = vgl_rc_class_of(len, g.b);
            m_acc += len;
        }
        vgl_wave_append<VGL_RC_N>(want, (int32_t)e, cls, g.L.list, g.L.cap, cnt + KT_TAIL);
    }
    vgl_wave_flush_add(cnt + KT_M, m_acc);
}
// a team per frontier edge
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ktruss_peel(const int32_t *edges, int32_t n, kt_graph g, int32_t k, int32_t s, unsigned long long *cnt)
{
    using T = vgl_rc_team<CLS>;
    int64_t m_acc = 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        const int32_t e = has ? edges[i] : 0;
        kt_rows r{0, 0, 0, 0};
        if (has) r = kt_rows_of(e, g);
        kt_expand(has, e, r, T::lane(), T::LANES, k, s, g, cnt + KT_TAIL, m_acc);
    }
    vgl_wave_flush_add(cnt + KT_M, m_acc);
}
// the peel stopped at k_limit: what is still alive gets k_limit
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_ktruss_fill_limit(int32_t ne, const int32_t *stamp, int32_t k_limit, int32_t *truss)
{
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < ne; e += (int64_t)gridDim.x * VGL_BLOCK)
        if (stamp[e] == 0) truss[e] = k_limit;
}

}  // namespace

extern "C" {

int vgl_hip_ktruss_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int64_t *undirected_edges)
{
    if (!c || !g) VGL_FAIL("ktruss_prepare: null argument");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("ktruss_prepare: graph handle must own all rows (the k-truss decomposition has no sharded form)");
    const vgl_simple_cache *kt = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_edge_ids(c, g, &kt, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    if (undirected_edges) *undirected_edges = kt->ne;
    return 0;
}

int vgl_hip_ktruss_run(vgl_hip_ctx *c, vgl_hip_graph *g, int32_t k_limit, int32_t *d_edge_u, int32_t *d_edge_v, int32_t *d_truss, int32_t *d_support,
                       vgl_hip_ktruss_stats *stats)
{
    if (!c || !g) VGL_FAIL("ktruss_run: null argument");
    if (!d_truss) VGL_FAIL("ktruss_run: d_truss must not be NULL");
    if ((d_edge_u == nullptr) != (d_edge_v == nullptr)) VGL_FAIL("ktruss_run: d_edge_u and d_edge_v go together (both or neither)");
    if (k_limit < 0 || k_limit == 1) VGL_FAIL("ktruss_run: k_limit must be 0 (the whole decomposition) or at least 2");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("ktruss_run: graph handle must own all rows (the k-truss decomposition has no sharded form)");
    const vgl_simple_cache *kt = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_edge_ids(c, g, &kt, &built));
    hipStream_t st = c->stream;
    vgl_hip_ktruss_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    out.undirected_edges = kt->ne;
    if (kt->ne == 0) {
        if (stats) *stats = out;
        return 0;
    }
    const int32_t ne = (int32_t)kt->ne;
    if (d_edge_u) {
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_u, kt->eu, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_v, kt->ev, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
    }

    // scratch of the call, all of it drawn before the loops: working supports, stamps, the class lists, the counters
    vgl_dev<int32_t> sup, stamp, lists;
    vgl_dev<unsigned long long> cnt;
    VGL_TRY(sup.alloc(st, (size_t)ne));
    VGL_TRY(stamp.alloc(st, (size_t)ne));
    VGL_TRY(lists.alloc(st, (size_t)ne * VGL_RC_N));
    VGL_TRY(cnt.alloc(st, KT_NCNT));
    VGL_HIP_TRY(hipMemsetAsync(stamp, 0, sizeof(int32_t) * (size_t)ne, st));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * KT_NCNT, st));

    kt_graph kg;
    kg.rowptr = kt->csr.rowptr; kg.adj = kt->csr.adj; kg.deg = kt->csr.deg;
    kg.eid = kt->eid; kg.eu = kt->eu; kg.ev = kt->ev;
    kg.sup = sup; kg.stamp = stamp; kg.truss = d_truss;
    kg.b = vgl_rc_env_bounds(c, "VGL_KTRUSS_SHORT", "VGL_KTRUSS_WAVE");
    for (int k_ = 0; k_ < VGL_RC_N; k_++) kg.L.list[k_] = lists.p + (size_t)ne * k_;
    kg.L.cap = ne;

    vgl_rc_window w;                             // the edges of the step: [head, tail) of the class lists
    int64_t m_cum = 0;
    // the one host-visible read of a step: the counters through the pinned mirror; the lists' new tails
    auto read = [&]() -> int {
        VGL_TRY(vgl_publish_counters(c, "ktruss_publish", cnt, KT_NCNT));
        VGL_TRY(w.advance(c->h_counters + KT_TAIL, ne, "ktruss_run: internal error (an edge list ran past its end)"));
        m_cum = c->h_counters[KT_M];
        return 0;
    };
    // a launch per class that has edges in [head, tail): the support pass and the peel have the same grids
    const int64_t cap[VGL_RC_N] = {KT_MAX_GRID, KT_MAX_GRID, KT_MAX_GRID};
    auto per_class = [&](const char *const *slot, auto k_short, auto k_wave, auto k_wg, auto... args) -> int {
        const int32_t *const edges[VGL_RC_N] = {kg.L.list[0] + w.head[0], kg.L.list[1] + w.head[1], kg.L.list[2] + w.head[2]};
        return vgl_rc_launch_trio(c, slot, w, cap, k_short, k_wave, k_wg, edges, kg, args...);
    };
    const char *const sup_slot[VGL_RC_N] = {"ktruss_sup_short", "ktruss_sup_wave", "ktruss_sup_wg"};
    const char *const peel_slot[VGL_RC_N] = {"ktruss_short", "ktruss_wave", "ktruss_wg"};

    // ---- the initial supports ----
    {
        vgl_timed_launch tl(c, "ktruss_classify");
        hipLaunchKernelGGL(vgl_k_ktruss_classify, dim3(vgl_grid(ne, VGL_BLOCK, KT_MAX_GRID)), dim3(VGL_BLOCK), 0, st, ne, kg, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(read());
    if (w.total() != ne) VGL_FAIL("ktruss_run: internal error (the classes do not add up to the edges)");
    VGL_TRY(per_class(sup_slot, vgl_k_ktruss_sup<VGL_RC_SHORT>, vgl_k_ktruss_sup<VGL_RC_WAVE>, vgl_k_ktruss_sup<VGL_RC_WG>, cnt.p));
    VGL_HIP_TRY(hipMemsetAsync(cnt.p + KT_TAIL, 0, sizeof(unsigned long long) * VGL_RC_N, st));      // the lists are the peel's from here on
    w = vgl_rc_window{};
    VGL_TRY(read());
    out.triangles = c->h_counters[KT_SUM] / 3;
    out.support_elements = c->h_counters[KT_WALK];
    out.max_support = (int32_t)c->h_counters[KT_MAXSUP];
    if (c->h_counters[KT_SUM] % 3 != 0) VGL_FAIL("ktruss_run: internal error (the supports do not add up to a multiple of three)");
    if (d_support) VGL_HIP_TRY(hipMemcpyAsync(d_support, sup, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));

    // ---- the peel ----
    int32_t k = 0, rounds = 0, s = 0;            // s: the sequence number of the current frontier (the stamps of its edges)
    int64_t subs = 0;
    bool limited = false;
    for (;;) {
        if (w.live() == 0) {                                                 // ---- k change ----
            if (w.total() == ne) break;
            VGL_HIP_TRY(hipMemsetAsync(cnt.p + KT_K, 0x7F, sizeof(unsigned long long), st));      // KT_NO_K
            {
                vgl_timed_launch tl(c, "ktruss_scan");
                hipLaunchKernelGGL(vgl_k_ktruss_min, dim3(vgl_grid(ne, VGL_BLOCK, 4096)), dim3(VGL_BLOCK), 0, st, ne, (const int32_t *)sup.p, (const int32_t *)stamp.p, cnt.p);
            }
            {
                vgl_timed_launch tl(c, "ktruss_scan");
                hipLaunchKernelGGL(vgl_k_ktruss_scan, dim3(vgl_grid(ne, VGL_BLOCK, 4096)), dim3(VGL_BLOCK), 0, st, ne, kg, s + 1, k_limit, cnt.p);
            }
            VGL_HIP_TRY(hipGetLastError());
            VGL_TRY(read());
            const int64_t m = c->h_counters[KT_K];
            if (m == KT_NO_K) VGL_FAIL("ktruss_run: internal error (edges are left but none is alive)");
            if (m < 0 || m + 2 <= k) VGL_FAIL("ktruss_run: internal error (the smallest remaining support is below the finished level)");
            if (k_limit > 0 && m + 2 >= k_limit) { limited = true; break; }
            k = (int32_t)m + 2;
            s++;
            rounds++;
            if (w.live() == 0) VGL_FAIL("ktruss_run: internal error (the level of the smallest remaining support is empty)");
            continue;
        }
        // ---- one sub-round: a launch per class that has edges, then the read ----
        if (s == INT_MAX) VGL_FAIL("ktruss_run: more than 2^31 sub-rounds");
        VGL_TRY(per_class(peel_slot, vgl_k_ktruss_peel<VGL_RC_SHORT>, vgl_k_ktruss_peel<VGL_RC_WAVE>, vgl_k_ktruss_peel<VGL_RC_WG>, k, s, cnt.p));
        VGL_TRY(read());
        s++;
        subs++;
    }
    if (limited) {
        hipLaunchKernelGGL(vgl_k_ktruss_fill_limit, dim3(vgl_grid(ne, VGL_BLOCK, 4096)), dim3(VGL_BLOCK), 0, st, ne, (const int32_t *)stamp.p, k_limit, d_truss);
        VGL_HIP_TRY(hipGetLastError());
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.max_truss = limited ? k_limit : k;
    out.rounds = rounds;
    out.sub_rounds = subs;
    out.peel_elements = m_cum;
    out.algorithmic_bytes = 28 * (int64_t)ne + 4 * (out.support_elements + out.peel_elements);
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
