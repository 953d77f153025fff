// kcore.hip -- k-core decomposition (core numbers, degeneracy, undirected degrees) of the simple undirected graph underlying the stored outgoing CSR.
// The contract is written out in include/vgl_hip.h; DESIGN section 15 has the schedule, the kernel resources and the bytes model.
//
// Prepare (once per graph, cached on the handle): the symmetric simple CSR of simple.hip (vgl_simple_ensure_csr), shared with ktruss and msf.
// degree = row length.
//
// Peel (level-synchronous; deg = a working copy of the degrees; a vertex is alive while deg > the last finished k):
//   k change   k = min over the alive vertices of deg (a device reduction: never a walk through empty shells); the alive vertices with deg <= k are
//              the first frontier of k.
//   sub-round  an expanded vertex v gets core[v] = k; for every entry u of its row with deg[u] > k:  old = atomicSub(&deg[u], 1);  old == k + 1: this
//              thread appends u to the next frontier (deg[u] crosses k + 1 -> k once and never comes back: below);  old <= k: the decrement is put back.
// A vertex enters a frontier exactly once, so the frontiers are consecutive segments [head, tail) of one list per row class and nothing is ever
// cleared or swapped.  Appends are aggregated: one returning atomic per wave and class (ballot + popcount).  Rows are split by length: short
// (<= VGL_KCORE_SHORT: 8 lanes per row), wave (<= VGL_KCORE_WAVE: one wavefront), workgroup (longer: one workgroup per VGL_KCORE_CHUNK entries).
// Small frontiers (<= 2048 vertices, <= VGL_KCORE_SMALL entries) run in vgl_k_kcore_small: ONE workgroup that loops over sub-rounds -- and over k
// changes while the vertices to scan are few (the whole graph, or the compacted list of the alive ones) -- until the work grows past the bound
// or the graph is exhausted, and reports through the pinned mirror what it did.  No cooperative launch, no workgroup waits for another.
// The host reads the pinned mirror once per sub-round of the large path (list tails, entry total, k); no allocation inside the loop.
#include "vgl_simple.h"
#include "vgl_rowclass.h"
#include <cstring>
#include <algorithm>
#include <climits>

namespace {

constexpr int KC_SMALL_THREADS = 1024;
constexpr int KC_SMALL_F = 2048;                // vertices of a frontier the one-workgroup kernel takes
constexpr int KC_SMALL_SCAN = 65536;            // vertices it scans itself on a k change (64 per thread)
constexpr int64_t KC_NO_K = 0x7F7F7F7F7F7F7F7Fll;      // "no alive vertex" in KC_K (a byte pattern: one memset arms the min kernel)
// device counters of a run (cumulative) and their slots in the pinned mirror
enum {
    KC_TAIL = 0,        // + class: entries appended to the class list so far
    KC_M = 3,           // row lengths of the appended vertices, summed = entries walked once they are all expanded
    KC_K = 4,           // the min kernel's result; published: the current (or last finished) k
    KC_ALIVE = 5,       // length of the compacted list of alive vertices
    KC_HEAD = 6,        // + class (mirror only, small kernel): the frontier it leaves starts here
    KC_CUR_M = 9,       // (mirror only, small kernel) entries of the frontier it leaves
    KC_ROUNDS = 10, KC_SUBS = 11, KC_STATE = 12,      // (mirror only, small kernel) k changes and sub-rounds it ran, why it ended
    KC_NCNT = 16
};
enum { KC_ST_BIG = 0, KC_ST_NEED_K = 1, KC_ST_DONE = 2, KC_ST_LIMIT = 3 };
static_assert(KC_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

struct kc_lists { int32_t *list[VGL_RC_N]; int32_t cap; };      // one list per class, `cap` entries each
struct kc_graph {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    int32_t *deg;                // working degrees
    int32_t *core;
    vgl_rc_bounds b;
    kc_lists L;
};

// ---- the peel: shared device pieces ----
// (appends: vgl_wave_append, one returning atomic per wave and class; tail: the three cumulative list lengths, in global memory or in LDS)
// One adjacency entry u of a vertex expanded at level k (active = this lane holds one).  deg[u] crosses k + 1 -> k exactly once: while it is above k
// it only falls; once it is at or below k every decrement that lands sees old <= k and is put back, so the value never returns to k + 1 and the
// append below happens in one thread.  A stale deg[u] can only be too large (the pre-check reads at device scope anyway), which costs an atomic.
__device__ __forceinline__ void kc_relax(bool active, int32_t u, int32_t k, const kc_graph &g, unsigned long long *tail, int64_t &m_acc)
{
    bool want = false;
    int cls = 0;
    if (active && vgl_load_agent(g.deg + u) > k) {
        const int32_t old = atomicSub(g.deg + u, 1);
        if (old == k + 1) {
            const int64_t len = g.rowptr[u + 1] - g.rowptr[u];
            want = true;
            cls = vgl_rc_class_of(len, g.b);
            m_acc += len;
        } else if (old <= k) atomicAdd(g.deg + u, 1);
    }
    vgl_wave_append<VGL_RC_N>(want, u, cls, g.L.list, g.L.cap, tail);
}
// the entries [lo, hi) of one row, `stride` lanes of which this is lane `li`; uniform over the wave as long as every lane of the wave calls
__device__ __forceinline__ void kc_walk(int64_t lo, int64_t hi, int li, int stride, int32_t k, const kc_graph &g, unsigned long long *tail, int64_t &m_acc)
{
    int64_t e = lo + li;
    while (__any(e < hi)) {
        const bool active = e < hi;
        const int32_t u = active ? g.adj[e] : 0;
        kc_relax(active, u, k, g, tail, m_acc);
        e += stride;
    }
}

// ---- the peel: large path ----
// cnt[KC_K] = min(deg) over the alive vertices of the scan domain (ids == nullptr: every vertex); alive: deg > k_prev
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_kcore_min(const int32_t *ids, int32_t n, const int32_t *deg, int32_t k_prev, unsigned long long *cnt)
{
    int m = INT_MAX;
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t d = deg[ids ? ids[i] : (int32_t)i];
        if (d > k_prev) m = min(m, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
    if (vgl_lane() == 0 && m != INT_MAX) atomicMin(cnt + KC_K, (unsigned long long)m);
}
// the first frontier of k = cnt[KC_K]: the alive vertices of the domain with deg <= k (nothing when no vertex is alive or k has reached k_limit)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_kcore_scan(const int32_t *ids, int32_t n, kc_graph g, int32_t k_prev, int32_t k_limit, unsigned long long *cnt)
{
    const unsigned long long k64 = cnt[KC_K];
    if (k64 == (unsigned long long)KC_NO_K || (k_limit > 0 && k64 >= (unsigned long long)k_limit)) return;
    const int32_t k = (int32_t)k64;
    int64_t m_acc = 0;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < n; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        bool want = false;
        int cls = 0;
        int32_t v = 0;
        if (i < n) {
            v = ids ? ids[i] : (int32_t)i;
            const int32_t d = g.deg[v];
            if (d > k_prev && d <= k) {
                const int64_t len = g.rowptr[v + 1] - g.rowptr[v];
                want = true;
                cls = vgl_rc_class_of(len, g.b);
                m_acc += len;
            }
        }
        vgl_wave_append<VGL_RC_N>(want, v, cls, g.L.list, g.L.cap, cnt + KC_TAIL);
    }
    vgl_wave_flush_add(cnt + KC_M, m_acc);
}
// the alive vertices, compacted (once, when few are left: the scans of the dense tail then read this list and not V degrees)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_kcore_compact(int32_t V, const int32_t *deg, int32_t k_prev, int32_t *alive, int32_t cap, unsigned long long *cnt)
{
    kc_lists L;
    L.list[0] = L.list[1] = L.list[2] = alive;
    L.cap = cap;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < V; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t v = base + threadIdx.x;
        vgl_wave_append<VGL_RC_N>(v < V && deg[v] > k_prev, (int32_t)v, 0, L.list, L.cap, cnt + KC_ALIVE);
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_kcore_short(kc_graph g, const int32_t *rows, int32_t n, int32_t k, unsigned long long *cnt)
{
    const int64_t i = ((int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x) / VGL_RC_G;
    const int gi = threadIdx.x & (VGL_RC_G - 1);
    int64_t lo = 0, hi = 0, m_acc = 0;
    if (i < n) {
        const int32_t v = rows[i];
        lo = g.rowptr[v]; hi = g.rowptr[v + 1];
        if (gi == 0) g.core[v] = k;
    }
    kc_walk(lo, hi, gi, VGL_RC_G, k, g, cnt + KC_TAIL, m_acc);
    vgl_wave_flush_add(cnt + KC_M, m_acc);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_kcore_wave(kc_graph g, const int32_t *rows, int32_t n, int32_t k, unsigned long long *cnt)
{
    const int64_t i = (int64_t)blockIdx.x * VGL_WAVES + vgl_wave();
    if (i >= n) return;                                               // (uniform over the wave)
    const int32_t v = rows[i];
    int64_t m_acc = 0;
    if (vgl_lane() == 0) g.core[v] = k;
    kc_walk(g.rowptr[v], g.rowptr[v + 1], vgl_lane(), 64, k, g, cnt + KC_TAIL, m_acc);
    vgl_wave_flush_add(cnt + KC_M, m_acc);
}
// workgroup (row blockIdx.x, piece blockIdx.y of its chunks): a workgroup past the end of its row has nothing to do
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_kcore_wg(kc_graph g, const int32_t *rows, vgl_rc_chunks ch, int32_t k, unsigned long long *cnt)
{
    const int32_t v = rows[blockIdx.x];
    int64_t lo, hi;
    const bool any = ch.range(g.rowptr[v], g.rowptr[v + 1], blockIdx.y, &lo, &hi);
    if (blockIdx.y == 0 && threadIdx.x == 0) g.core[v] = k;
    if (!any) return;                                                 // (uniform over the workgroup)
    int64_t m_acc = 0;
    kc_walk(lo, hi, (int)threadIdx.x, VGL_BLOCK, k, g, cnt + KC_TAIL, m_acc);
    vgl_wave_flush_add(cnt + KC_M, m_acc);
}
// the peel stopped at k_limit: what is still alive gets k_limit
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_kcore_fill_limit(int32_t V, const int32_t *deg, int32_t k_last, int32_t k_limit, int32_t *core)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK)
        if (deg[v] > k_last) core[v] = k_limit;
}

// ---- the peel: small frontiers, ONE workgroup ----
// Entry: the frontier of level k is [head[c], cnt[KC_TAIL + c]) of the class lists and has cur_m entries; it may be empty, k then being the last
// finished level (-1: none yet).  dom_n > 0: on a k change this workgroup scans the domain (dom_ids == nullptr: the vertices 0 .. dom_n - 1) itself;
// dom_n == 0: it ends there and the host runs the scan kernels.  It ends (state in the mirror) when the next frontier is too large for it
// (KC_ST_BIG: the lists hold it, as after a sub-round of the large path), a k change is not its to make (KC_ST_NEED_K), no vertex is alive
// (KC_ST_DONE) or k has reached k_limit (KC_ST_LIMIT).  Every turn of the loop expands a frontier or changes k, so it ends after at most 2 V turns.
// Values other threads of the workgroup wrote are read at device scope (degrees, list entries), never from a line this CU may have cached.
__global__ __launch_bounds__(KC_SMALL_THREADS) void vgl_k_kcore_small(kc_graph g, const int32_t *dom_ids, int32_t dom_n, int64_t head0, int64_t head1, int64_t head2,
                                                                      int64_t cur_m, int32_t k, int32_t k_limit, int64_t cap_m, unsigned long long *cnt,
                                                                      volatile int64_t *host, int64_t seq)
{
    constexpr int NT = KC_SMALL_THREADS, NW = NT / 64;
    __shared__ unsigned long long s_tail[VGL_RC_N];
    __shared__ unsigned long long s_m;
    __shared__ int s_min;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t head[VGL_RC_N] = {head0, head1, head2};
    int64_t rounds = 0, subs = 0, m_total = 0;
    int state = KC_ST_BIG;
    if (tid < VGL_RC_N) s_tail[tid] = cnt[KC_TAIL + tid];
    if (tid == 0) s_m = 0;
    for (;;) {
        __syncthreads();                                              // the lists, s_tail and s_m = 0 are in place; s_min has been read
        int64_t tail[VGL_RC_N];
        int64_t F = 0;
#pragma unroll
        for (int c = 0; c < VGL_RC_N; c++) { tail[c] = (int64_t)s_tail[c]; F += tail[c] - head[c]; }
        int64_t m_acc = 0;
        if (F == 0) {                                                 // ---- k change ----
            if (dom_n <= 0) { state = KC_ST_NEED_K; break; }
            if (tid == 0) s_min = INT_MAX;
            __syncthreads();
            int m = INT_MAX;
            for (int i = tid; i < dom_n; i += NT) {
                const int32_t d = vgl_load_agent(g.deg + (dom_ids ? dom_ids[i] : i));
                if (d > k) m = min(m, d);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
            if (lane == 0 && m != INT_MAX) atomicMin(&s_min, m);
            __syncthreads();
            const int kn = s_min;
            if (kn == INT_MAX) { state = KC_ST_DONE; break; }
            if (k_limit > 0 && kn >= k_limit) { state = KC_ST_LIMIT; break; }
            for (int base = 0; base < dom_n; base += NT) {            // (uniform over the workgroup)
                const int i = base + tid;
                bool want = false;
                int cls = 0;
                int32_t v = 0;
                if (i < dom_n) {
                    v = dom_ids ? dom_ids[i] : i;
                    const int32_t d = vgl_load_agent(g.deg + v);
                    if (d > k && d <= kn) {
                        const int64_t len = g.rowptr[v + 1] - g.rowptr[v];
                        want = true;
                        cls = vgl_rc_class_of(len, g.b);
                        m_acc += len;
                    }
                }
                vgl_wave_append<VGL_RC_N>(want, v, cls, g.L.list, g.L.cap, s_tail);
            }
            k = kn;
            rounds++;
        } else {                                                      // ---- one sub-round ----
            if (F > KC_SMALL_F || cur_m > cap_m) { state = KC_ST_BIG; break; }
            {                                                         // short rows: 8 lanes each
                const int64_t n = tail[VGL_RC_SHORT] - head[VGL_RC_SHORT];
                for (int64_t i0 = 0; i0 < n; i0 += NT / VGL_RC_G) {       // (uniform over the workgroup)
                    const int64_t i = i0 + tid / VGL_RC_G;
                    int64_t lo = 0, hi = 0;
                    if (i < n) {
                        const int32_t v = vgl_load_agent(g.L.list[VGL_RC_SHORT] + head[VGL_RC_SHORT] + i);
                        lo = g.rowptr[v]; hi = g.rowptr[v + 1];
                        if ((tid & (VGL_RC_G - 1)) == 0) g.core[v] = k;
                    }
                    kc_walk(lo, hi, tid & (VGL_RC_G - 1), VGL_RC_G, k, g, s_tail, m_acc);
                }
            }
            {                                                         // longer rows: a wavefront each (cur_m <= cap_m bounds them)
                const int64_t n1 = tail[VGL_RC_WAVE] - head[VGL_RC_WAVE], n = n1 + tail[VGL_RC_WG] - head[VGL_RC_WG];
                for (int64_t j = wave; j < n; j += NW) {              // (uniform over the wave)
                    const int32_t v = j < n1 ? vgl_load_agent(g.L.list[VGL_RC_WAVE] + head[VGL_RC_WAVE] + j) : vgl_load_agent(g.L.list[VGL_RC_WG] + head[VGL_RC_WG] + (j - n1));
                    if (lane == 0) g.core[v] = k;
                    kc_walk(g.rowptr[v], g.rowptr[v + 1], lane, 64, k, g, s_tail, m_acc);
                }
            }
#pragma unroll
            for (int c = 0; c < VGL_RC_N; c++) head[c] = tail[c];
            subs++;
        }
        m_acc = vgl_wave_reduce_add(m_acc);
        if (lane == 0 && m_acc) atomicAdd(&s_m, (unsigned long long)m_acc);
        __syncthreads();                                              // every append and every add to s_m has landed
        cur_m = (int64_t)s_m;
        m_total += cur_m;
        __syncthreads();
        if (tid == 0) s_m = 0;
    }
    // (the breaks above are uniform over the workgroup and come right after a barrier: nobody is still appending)
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < VGL_RC_N; c++) {
            cnt[KC_TAIL + c] = s_tail[c];
            host[KC_TAIL + c] = (int64_t)s_tail[c];
            host[KC_HEAD + c] = head[c];
        }
        const unsigned long long m_cum = cnt[KC_M] + (unsigned long long)m_total;
        cnt[KC_M] = m_cum;
        host[KC_M] = (int64_t)m_cum;
        host[KC_K] = k;
        host[KC_CUR_M] = cur_m;
        host[KC_ROUNDS] = rounds;
        host[KC_SUBS] = subs;
        host[KC_STATE] = state;
        __threadfence_system();
        host[C_NSLOTS] = seq;
        __threadfence_system();
    }
}

// the host side of one run: where the frontier is, what has been counted
struct kc_run {
    vgl_hip_ctx *c;
    kc_graph g;
    unsigned long long *cnt;
    vgl_rc_window w;                     // the frontier: [head, tail) of the class lists
    int64_t m_cum = 0, cur_m = 0;        // entries of every frontier so far / of the current one
    int32_t k = -1;                      // the current level, or the last finished one while the frontier is empty
    int32_t rounds = 0;
    int64_t subs = 0;

    // the one host-visible read of a sub-round of the large path: list tails and entry total
    int read()
    {
        VGL_TRY(vgl_publish_counters(c, "kcore_publish", cnt, KC_NCNT));
        VGL_TRY(w.advance(c->h_counters + KC_TAIL, g.L.cap, "kcore_run: internal error (a frontier list ran past its end)"));
        cur_m = c->h_counters[KC_M] - m_cum;
        m_cum = c->h_counters[KC_M];
        return 0;
    }
};

}  // namespace

extern "C" {

int vgl_hip_kcore_prepare(vgl_hip_ctx *c, vgl_hip_graph *g)
{
    if (!c || !g) VGL_FAIL("kcore_prepare: null argument");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("kcore_prepare: graph handle must own all rows (the k-core decomposition has no sharded form)");
    const vgl_simple_cache *k = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_csr(c, g, &k, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_kcore_run(vgl_hip_ctx *c, vgl_hip_graph *g, int32_t k_limit, int32_t *d_core, int32_t *d_degree, vgl_hip_kcore_stats *stats)
{
    if (!c || !g) VGL_FAIL("kcore_run: null argument");
    if (!d_core) VGL_FAIL("kcore_run: d_core must not be NULL");
    if (k_limit < 0) VGL_FAIL("kcore_run: k_limit must not be negative");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("kcore_run: graph handle must own all rows (the k-core decomposition has no sharded form)");
    const vgl_simple_cache *sc = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_csr(c, g, &sc, &built));
    const vgl_simple_csr *kc = &sc->csr;
    const int32_t V = g->V;
    hipStream_t st = c->stream;
    const int64_t chunk_env = vgl_rc_env_chunk(c, "VGL_KCORE_CHUNK");
    const int64_t small_m = vgl_env_int(c, "VGL_KCORE_SMALL", 8192, 0, 1 << 20);
    vgl_hip_kcore_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    out.undirected_edges = kc->nnz / 2;
    out.max_degree = kc->max_deg;
    if (V == 0) {
        if (stats) *stats = out;
        return 0;
    }
    if (d_degree) VGL_HIP_TRY(hipMemcpyAsync(d_degree, kc->deg, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToDevice, st));

    // scratch of the call, all of it drawn before the loop: working degrees, the class lists, the compacted alive list, the counters
    vgl_dev<int32_t> deg, lists, alive;
    vgl_dev<unsigned long long> cnt;
    VGL_TRY(deg.alloc(st, (size_t)V));
    VGL_TRY(lists.alloc(st, (size_t)V * VGL_RC_N));
    VGL_TRY(alive.alloc(st, (size_t)std::min<int32_t>(V, KC_SMALL_SCAN)));
    VGL_TRY(cnt.alloc(st, KC_NCNT));
    VGL_HIP_TRY(hipMemcpyAsync(deg, kc->deg, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToDevice, st));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * KC_NCNT, st));

    kc_run r;
    r.c = c;
    r.cnt = cnt;
    r.g.rowptr = kc->rowptr; r.g.adj = kc->adj; r.g.deg = deg; r.g.core = d_core;
    r.g.b = vgl_rc_env_bounds(c, "VGL_KCORE_SHORT", "VGL_KCORE_WAVE");
    for (int k_ = 0; k_ < VGL_RC_N; k_++) r.g.L.list[k_] = lists.p + (size_t)V * k_;
    r.g.L.cap = V;
    const vgl_rc_chunks ch = vgl_rc_chunks::of(chunk_env, kc->max_deg);      // grid.y of the workgroup kernel: at most VGL_RC_MAX_CHUNKS
    const int32_t *dom_ids = nullptr;                                 // the scan domain: every vertex, or the compacted alive list
    int32_t dom_n = V;
    bool limited = false;
    const char *const slot[VGL_RC_N] = {"kcore_short", "kcore_wave", "kcore_wg"};

    // one launch of the one-workgroup kernel and the read of what it did
    auto small = [&]() -> int {
        const int64_t seq = vgl_next_seq(c);
        {
            vgl_timed_launch tl(c, "kcore_small");
            hipLaunchKernelGGL(vgl_k_kcore_small, dim3(1), dim3(KC_SMALL_THREADS), 0, st, r.g, dom_ids, dom_n <= KC_SMALL_SCAN ? dom_n : 0, r.w.head[0], r.w.head[1], r.w.head[2], r.cur_m,
                               r.k, k_limit, small_m, cnt.p, (volatile int64_t *)c->h_counters, seq);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(vgl_wait_counters(c, seq));
        const int64_t *h = c->h_counters;
        for (int k_ = 0; k_ < VGL_RC_N; k_++) {
            r.w.head[k_] = h[KC_HEAD + k_];
            r.w.tail[k_] = h[KC_TAIL + k_];
            if (r.w.head[k_] < 0 || r.w.tail[k_] < r.w.head[k_] || r.w.tail[k_] > V) VGL_FAIL("kcore_run: internal error (a frontier list ran past its end)");
        }
        r.m_cum = h[KC_M];
        r.cur_m = h[KC_CUR_M];
        r.k = (int32_t)h[KC_K];
        r.rounds += (int32_t)h[KC_ROUNDS];
        r.subs += h[KC_SUBS];
        return (int)h[KC_STATE];
    };

    for (;;) {
        const int64_t F = r.w.live();
        if (F == 0) {                                                 // ---- k change ----
            const int64_t left = V - r.w.total();
            if (left == 0) break;
            if (small_m > 0 && !dom_ids && V > KC_SMALL_SCAN && left <= KC_SMALL_SCAN) {      // few are left: from now on the scans read their list
                {
                    vgl_timed_launch tl(c, "kcore_scan");
                    hipLaunchKernelGGL(vgl_k_kcore_compact, dim3(vgl_grid(V, VGL_BLOCK, 4096)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)deg.p, r.k, alive.p, KC_SMALL_SCAN, cnt.p);
                }
                VGL_HIP_TRY(hipGetLastError());
                dom_ids = alive;
                dom_n = (int32_t)left;                                // (alive = not yet in a list: the kernel appends exactly these)
            }
            if (small_m > 0 && dom_n <= KC_SMALL_SCAN) {
                const int state = small();
                if (state == KC_ST_DONE) break;
                if (state == KC_ST_LIMIT) { limited = true; break; }
                if (state == KC_ST_NEED_K) VGL_FAIL("kcore_run: internal error (the one-workgroup kernel refused a scan it was given)");
                continue;
            }
            VGL_HIP_TRY(hipMemsetAsync(cnt.p + KC_K, 0x7F, sizeof(unsigned long long), st));      // KC_NO_K
            {
                vgl_timed_launch tl(c, "kcore_scan");
                hipLaunchKernelGGL(vgl_k_kcore_min, dim3(vgl_grid(dom_n, VGL_BLOCK, 4096)), dim3(VGL_BLOCK), 0, st, dom_ids, dom_n, (const int32_t *)deg.p, r.k, cnt.p);
            }
            {
                vgl_timed_launch tl(c, "kcore_scan");
                hipLaunchKernelGGL(vgl_k_kcore_scan, dim3(vgl_grid(dom_n, VGL_BLOCK, 4096)), dim3(VGL_BLOCK), 0, st, dom_ids, dom_n, r.g, r.k, k_limit, cnt.p);
            }
            VGL_HIP_TRY(hipGetLastError());
            VGL_TRY(r.read());
            const int64_t kn = c->h_counters[KC_K];
            if (kn == KC_NO_K) VGL_FAIL("kcore_run: internal error (vertices are left but none is alive)");
            if (k_limit > 0 && kn >= k_limit) { limited = true; break; }
            r.k = (int32_t)kn;
            r.rounds++;
            if (r.w.live() == 0) VGL_FAIL("kcore_run: internal error (the shell of the smallest remaining degree is empty)");
            continue;
        }
        if (small_m > 0 && F <= KC_SMALL_F && r.cur_m <= small_m) {   // ---- small frontier: several sub-rounds in one workgroup ----
            const int state = small();
            if (state == KC_ST_DONE) break;
            if (state == KC_ST_LIMIT) { limited = true; break; }
            continue;
        }
        // ---- one sub-round of the large path: a launch per class that has rows, then the read ----
        VGL_TRY(vgl_rc_launch(c, slot, r.w, [&](int cls, int64_t n) {
            const int32_t *rows = r.g.L.list[cls] + r.w.head[cls];
            if (cls == VGL_RC_SHORT)
                hipLaunchKernelGGL(vgl_k_kcore_short, dim3(vgl_grid(n * VGL_RC_G, VGL_BLOCK, (int64_t)1 << 30)), dim3(VGL_BLOCK), 0, st, r.g, rows, (int32_t)n, r.k, cnt.p);
            else if (cls == VGL_RC_WAVE)
                hipLaunchKernelGGL(vgl_k_kcore_wave, dim3(vgl_grid(n, VGL_WAVES, (int64_t)1 << 30)), dim3(VGL_BLOCK), 0, st, r.g, rows, (int32_t)n, r.k, cnt.p);
            else
                hipLaunchKernelGGL(vgl_k_kcore_wg, dim3((unsigned)n, (unsigned)ch.nchunks), dim3(VGL_BLOCK), 0, st, r.g, rows, ch, r.k, cnt.p);
        }));
        VGL_TRY(r.read());
        r.subs++;
    }
    if (limited) {
        hipLaunchKernelGGL(vgl_k_kcore_fill_limit, dim3(vgl_grid(V, VGL_BLOCK, 4096)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)deg.p, r.k, k_limit, d_core);
        VGL_HIP_TRY(hipGetLastError());
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.degeneracy = limited ? k_limit : std::max(r.k, 0);
    out.rounds = r.rounds;
    out.sub_rounds = r.subs;
    out.edges_examined = r.m_cum;
    out.algorithmic_bytes = 20 * (int64_t)V + 8 * r.m_cum;
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
