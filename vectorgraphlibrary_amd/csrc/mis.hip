// mis.hip -- the lexicographically first maximal independent set (vertices) and maximal matching (edges) of the simple undirected graph underlying
// the stored outgoing CSR, under the order (key, id).  The contract is written out in include/vgl_hip.h; DESIGN section 22 has the rounds, the kernel
// resources and the bytes model.
//
// Both are the synchronous rounds of Blelloch, Fineman and Shun (SPAA 2012), which return what the sequential greedy algorithm returns.
//   MIS       state[v] = 0 undecided, +r IN since round r, -r OUT since round r.  Round r, the undecided rows, one kernel per row class (short: 8 lanes
//             per row, wave, workgroup): a lane looks at the entries w that come before v in the order -- the key is computed (or gathered from the
//             caller's array) first, state[w] only for those -- and keeps two bits: an earlier neighbour is IN since a round < r; an earlier neighbour
//             is undecided (0, or +-r: a decision of this very round).  The first bit: v is OUT.  Neither: v is IN.  Otherwise v is appended again.
//             One int32 array, no double buffer: a store of this launch reads as undecided whether or not it has landed.
//   matching  pass 1, the live rows per row class: best[v] = min over the entries whose far end is unmatched of (key(edge) << 32 | edge), a 64-bit
//             shuffle reduce per row group; a row without such an entry leaves for good, the others go to the candidate list.  Pass 2, the candidates
//             (their number is read from the device counter: no host read between the passes): edge e = best[v] is matched iff the far end holds the
//             same best; both ends write their mate, the lower end the edge's flag; the others are appended to the live ring of their class.
// The live lists are one ring per class of twice the class's rows (msf's scheme): a round reads [head, tail) and appends behind tail; appends are
// staged per wave in LDS (vgl_rc_stage).  One host read of the pinned mirror per round.  No cooperative launch, no grid barrier, no floating point.
#include "vgl_simple.h"
#include "vgl_rowclass.h"
#include <cstring>
#include <algorithm>
#include <climits>

namespace {

constexpr int64_t MIS_MAX_GRID = 2048;            // workgroups of a grid-stride kernel
constexpr unsigned long long MM_NONE = ~0ull;     // "no entry with an unmatched far end" in best
enum {
    MIS_TAIL = 0,       // + class: rows appended to the class ring so far (cumulative)
    MIS_IN = 3,         // vertices that went IN so far
    MIS_WALK = 4,       // row lengths of the live rows, summed over the rounds so far
    MIS_ROWS = 5,       // + class: rows per class
    MIS_NCNT = 8
};
enum {
    MM_TAIL = 0,        // + class: rows appended to the class ring so far (cumulative)
    MM_CAND = 3,        // rows appended to the candidate list so far (cumulative)
    MM_EDGES = 4,       // edges matched so far
    MM_WALK = 5,        // row lengths of the live rows of the first passes, summed over the rounds so far
    MM_ROWS = 6,        // + class: rows per class
    MM_NCNT = 9
};
static_assert(MIS_NCNT <= C_NSLOTS && MM_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

// the murmur3 finaliser: a bijection of uint32
__host__ __device__ inline uint32_t mis_fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
// key(i, seed) = fmix32(i ^ mix), mix = fmix32(seed + 0x9e3779b9); or the caller's array
struct mis_keys {
    const uint32_t *prio; uint32_t mix;
    __device__ __forceinline__ uint32_t of(int32_t i) const { return prio ? prio[i] : mis_fmix32((uint32_t)i ^ mix); }
};

// ---- the live lists: every vertex, by the length of its row ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mis_count(int32_t V, const int32_t *deg, vgl_rc_bounds b, unsigned long long *rows)
{
    int64_t n[VGL_RC_N] = {0, 0, 0};
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) n[vgl_rc_class_of(deg[v], b)]++;
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) vgl_wave_flush_add(rows + c, n[c]);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mis_fill(int32_t V, const int32_t *deg, vgl_rc_bounds b, vgl_rc_ring R0, vgl_rc_ring R1, vgl_rc_ring R2, unsigned long long *tail)
{
    const vgl_rc_ring R[VGL_RC_N] = {R0, R1, R2};
    vgl_rc_stage st[VGL_RC_N];
    vgl_rc_stage_open(st);
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < V; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t v = base + threadIdx.x;
        const int cls = v < V ? vgl_rc_class_of(deg[v], b) : -1;
#pragma unroll
        for (int c = 0; c < VGL_RC_N; c++) st[c].keep(cls == c, (int32_t)v, R[c], tail + c);
    }
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) st[c].flush(R[c], tail + c);
}

// ---- maximal independent set ----
struct mis_graph {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    mis_keys key;                // of the vertices
    int32_t *state;              // the signed round
};
// entry w of v's row in round r: 1 = w comes before v and is IN since an earlier round; 2 = w comes before v and is undecided; 0 otherwise
__device__ __forceinline__ int mis_look(const mis_graph &g, int32_t v, uint32_t kv, int32_t w, int32_t r)
{
    const uint32_t kw = g.key.of(w);
    if (kw > kv || (kw == kv && w >= v)) return 0;
    const int32_t s = g.state[w];
    if (s == 0 || s == r || s == -r) return 2;
    return s > 0 ? 1 : 0;
}
// the lane that speaks for row v (bits = the OR over the row) decides; true: v stays undecided
__device__ __forceinline__ bool mis_decide(const mis_graph &g, int32_t v, int bits, int32_t r, int64_t &in)
{
    if (bits & 1) { g.state[v] = -r; return false; }
    if (bits & 2) return true;
    g.state[v] = r;
    in++;
    return false;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mis_short(mis_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, int32_t r, unsigned long long *cnt)
{
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    const int gi = threadIdx.x & (VGL_RC_G - 1);
    int64_t walked = 0, in = 0;
    for (int64_t base = (int64_t)blockIdx.x * (VGL_BLOCK / VGL_RC_G); base < n; base += (int64_t)gridDim.x * (VGL_BLOCK / VGL_RC_G)) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x / VGL_RC_G;
        int32_t v = 0;
        uint32_t kv = 0;
        int64_t lo = 0, hi = 0;
        if (i < n) {
            v = R.rows[(head + (unsigned long long)i) % R.cap];
            kv = g.key.of(v);
            lo = g.rowptr[v]; hi = g.rowptr[v + 1];
        }
        int bits = 0;
        for (int64_t e = lo + gi; e < hi; e += VGL_RC_G) bits |= mis_look(g, v, kv, g.adj[e], r);
#pragma unroll
        for (int o = VGL_RC_G / 2; o > 0; o >>= 1) bits |= __shfl_xor(bits, o);
        bool again = false;
        if (gi == 0 && i < n) {
            walked += hi - lo;
            again = mis_decide(g, v, bits, r, in);
        }
        st[0].keep(again, v, R, cnt + MIS_TAIL + VGL_RC_SHORT);
    }
    st[0].flush(R, cnt + MIS_TAIL + VGL_RC_SHORT);
    vgl_wave_flush_add(cnt + MIS_WALK, walked);
    vgl_wave_flush_add(cnt + MIS_IN, in);
}
// a wavefront per row; the scan stops at the first earlier neighbour that is IN
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mis_wave(mis_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, int32_t r, unsigned long long *cnt)
{
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    const int lane = vgl_lane();
    int64_t walked = 0, in = 0;
    for (int64_t i = (int64_t)blockIdx.x * VGL_WAVES + vgl_wave(); i < n; i += (int64_t)gridDim.x * VGL_WAVES) {      // (uniform over the wave)
        const int32_t v = R.rows[(head + (unsigned long long)i) % R.cap];
        const uint32_t kv = g.key.of(v);
        const int64_t lo = g.rowptr[v], hi = g.rowptr[v + 1];
        int bits = 0;
        for (int64_t e = lo; e < hi; e += 64) {                       // (uniform over the wave)
            if (e + lane < hi) bits |= mis_look(g, v, kv, g.adj[e + lane], r);
            if (__any(bits & 1)) break;
        }
        bits = (__any(bits & 1) ? 1 : 0) | (__any(bits & 2) ? 2 : 0);
        bool again = false;
        if (lane == 0) {
            walked += hi - lo;
            again = mis_decide(g, v, bits, r, in);
        }
        st[0].keep(again, v, R, cnt + MIS_TAIL + VGL_RC_WAVE);
    }
    st[0].flush(R, cnt + MIS_TAIL + VGL_RC_WAVE);
    vgl_wave_flush_add(cnt + MIS_WALK, walked);
    vgl_wave_flush_add(cnt + MIS_IN, in);
}
// a workgroup per row
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mis_wg(mis_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, int32_t r, unsigned long long *cnt)
{
    __shared__ int s_bits;
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    int64_t walked = 0, in = 0;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {             // (uniform over the workgroup)
        if (threadIdx.x == 0) s_bits = 0;
        __syncthreads();
        const int32_t v = R.rows[(head + (unsigned long long)i) % R.cap];
        const uint32_t kv = g.key.of(v);
        const int64_t lo = g.rowptr[v], hi = g.rowptr[v + 1];
        int bits = 0;
        for (int64_t e = lo + threadIdx.x; e < hi; e += VGL_BLOCK) bits |= mis_look(g, v, kv, g.adj[e], r);
        bits = (__any(bits & 1) ? 1 : 0) | (__any(bits & 2) ? 2 : 0);
        if (vgl_lane() == 0 && bits) atomicOr(&s_bits, bits);
        __syncthreads();
        bits = s_bits;
        __syncthreads();
        bool again = false;
        if (threadIdx.x == 0) {
            walked += hi - lo;
            again = mis_decide(g, v, bits, r, in);
        }
        st[0].keep(again, v, R, cnt + MIS_TAIL + VGL_RC_WG);
    }
    st[0].flush(R, cnt + MIS_TAIL + VGL_RC_WG);
    vgl_wave_flush_add(cnt + MIS_WALK, walked);
    vgl_wave_flush_add(cnt + MIS_IN, in);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mis_finish(int32_t V, const int32_t *state, uint8_t *in_set)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) in_set[v] = state[v] > 0 ? 1 : 0;
}

// ---- maximal matching ----
struct mm_graph {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    const int32_t *eid;          // edge id of every adjacency slot
    mis_keys key;                // of the edges
    const int32_t *mate;
    unsigned long long *best;
};
__device__ __forceinline__ unsigned long long mm_wave_min(unsigned long long m)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
    return m;
}
// the smallest  key << 32 | edge  over the entries lo, lo + stride, ... < hi whose far end is unmatched
__device__ __forceinline__ unsigned long long mm_walk(int64_t lo, int64_t hi, int stride, const mm_graph &g)
{
    unsigned long long m = MM_NONE;
    for (int64_t i = lo; i < hi; i += stride)
        if (g.mate[g.adj[i]] < 0) {
            const int32_t e = g.eid[i];
            m = min(m, (unsigned long long)g.key.of(e) << 32 | (unsigned long long)(uint32_t)e);
        }
    return m;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mm_best_short(mm_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, vgl_rc_ring cand, unsigned long long *cnt)
{
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    const int gi = threadIdx.x & (VGL_RC_G - 1);
    int64_t walked = 0;
    for (int64_t base = (int64_t)blockIdx.x * (VGL_BLOCK / VGL_RC_G); base < n; base += (int64_t)gridDim.x * (VGL_BLOCK / VGL_RC_G)) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x / VGL_RC_G;
        int32_t v = 0;
        int64_t lo = 0, hi = 0;
        if (i < n) {
            v = R.rows[(head + (unsigned long long)i) % R.cap];
            lo = g.rowptr[v]; hi = g.rowptr[v + 1];
        }
        unsigned long long m = mm_walk(lo + gi, hi, VGL_RC_G, g);
#pragma unroll
        for (int o = VGL_RC_G / 2; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
        const bool lead = gi == 0 && i < n;
        if (lead) {
            walked += hi - lo;
            g.best[v] = m;
        }
        st[0].keep(lead && m != MM_NONE, v, cand, cnt + MM_CAND);
    }
    st[0].flush(cand, cnt + MM_CAND);
    vgl_wave_flush_add(cnt + MM_WALK, walked);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mm_best_wave(mm_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, vgl_rc_ring cand, unsigned long long *cnt)
{
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    const int lane = vgl_lane();
    int64_t walked = 0;
    for (int64_t i = (int64_t)blockIdx.x * VGL_WAVES + vgl_wave(); i < n; i += (int64_t)gridDim.x * VGL_WAVES) {      // (uniform over the wave)
        const int32_t v = R.rows[(head + (unsigned long long)i) % R.cap];
        const int64_t lo = g.rowptr[v], hi = g.rowptr[v + 1];
        const unsigned long long m = mm_wave_min(mm_walk(lo + lane, hi, 64, g));
        if (lane == 0) {
            walked += hi - lo;
            g.best[v] = m;
        }
        st[0].keep(lane == 0 && m != MM_NONE, v, cand, cnt + MM_CAND);
    }
    st[0].flush(cand, cnt + MM_CAND);
    vgl_wave_flush_add(cnt + MM_WALK, walked);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mm_best_wg(mm_graph g, vgl_rc_ring R, unsigned long long head, int32_t n, vgl_rc_ring cand, unsigned long long *cnt)
{
    __shared__ unsigned long long s_red[VGL_WAVES];
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    int64_t walked = 0;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {             // (uniform over the workgroup)
        const int32_t v = R.rows[(head + (unsigned long long)i) % R.cap];
        const int64_t lo = g.rowptr[v], hi = g.rowptr[v + 1];
        unsigned long long m = mm_wave_min(mm_walk(lo + threadIdx.x, hi, VGL_BLOCK, g));
        __syncthreads();
        if (vgl_lane() == 0) s_red[vgl_wave()] = m;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < VGL_WAVES; k++) m = min(m, s_red[k]);
        if (threadIdx.x == 0) {
            walked += hi - lo;
            g.best[v] = m;
        }
        st[0].keep(threadIdx.x == 0 && m != MM_NONE, v, cand, cnt + MM_CAND);
    }
    st[0].flush(cand, cnt + MM_CAND);
    vgl_wave_flush_add(cnt + MM_WALK, walked);
}
// pass 2 over the candidates [cand_head, cnt[MM_CAND]) of this round
struct mm_out { int32_t *mate, *round; uint8_t *in_matching; };
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mm_match(int32_t r, const unsigned long long *best, const int32_t *eu, const int32_t *ev, const int32_t *deg, vgl_rc_bounds b, mm_out out,
                                                             vgl_rc_ring cand, unsigned long long cand_head, vgl_rc_ring R0, vgl_rc_ring R1, vgl_rc_ring R2, unsigned long long *cnt)
{
    const vgl_rc_ring R[VGL_RC_N] = {R0, R1, R2};
    vgl_rc_stage st[VGL_RC_N];
    vgl_rc_stage_open(st);
    const int64_t n = (int64_t)(cnt[MM_CAND] - cand_head);
    int64_t matched = 0;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < n; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        int32_t v = 0;
        int cls = -1;
        if (i < n) {
            v = cand.rows[(cand_head + (unsigned long long)i) % cand.cap];
            const unsigned long long k = best[v];
            const int32_t e = (int32_t)(uint32_t)k;
            const int32_t lo = eu[e], hi = ev[e];
            const int32_t far = lo == v ? hi : lo;
            if (best[far] == k) {
                out.mate[v] = far;
                if (out.round) out.round[v] = r;
                if (v == lo) {
                    if (out.in_matching) out.in_matching[e] = 1;
                    matched++;
                }
            } else cls = vgl_rc_class_of(deg[v], b);
        }
#pragma unroll
        for (int c = 0; c < VGL_RC_N; c++) st[c].keep(cls == c, v, R[c], cnt + MM_TAIL + c);
    }
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) st[c].flush(R[c], cnt + MM_TAIL + c);
    vgl_wave_flush_add(cnt + MM_EDGES, matched);
}

// ---- host: the rings of a run ----
struct mis_lists {
    vgl_dev<int32_t> mem;
    vgl_rc_ring R[VGL_RC_N];
    vgl_rc_window w;
};
// every vertex into the ring of its class (cnt + tail0: the three tails; cnt + rows0: the three row counts); one host read
int mis_open_lists(vgl_hip_ctx *c, int32_t V, const int32_t *deg, vgl_rc_bounds b, unsigned long long *cnt, int tail0, int rows0, int ncnt, const char *slot_init, const char *slot_publish,
                   mis_lists *L)
{
    hipStream_t st = c->stream;
    {
        vgl_timed_launch tl(c, slot_init);
        hipLaunchKernelGGL(vgl_k_mis_count, dim3(vgl_grid(V, VGL_BLOCK, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, deg, b, cnt + rows0);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_publish_counters(c, slot_publish, cnt, ncnt));
    int64_t rows[VGL_RC_N], total = 0;
    for (int k = 0; k < VGL_RC_N; k++) {
        rows[k] = c->h_counters[rows0 + k];
        if (rows[k] < 0 || rows[k] > V) VGL_FAIL("mis: internal error (more rows in a class than vertices)");
        total += rows[k];
    }
    if (total != V) VGL_FAIL("mis: internal error (the classes do not add up to the vertices)");
    VGL_TRY(L->mem.alloc(st, (size_t)(2 * total)));
    int64_t off = 0;
    for (int k = 0; k < VGL_RC_N; k++) {
        L->R[k].rows = L->mem.p + off;
        L->R[k].cap = (uint32_t)(2 * rows[k]);
        off += 2 * rows[k];
        L->w.tail[k] = rows[k];
    }
    {
        vgl_timed_launch tl(c, slot_init);
        hipLaunchKernelGGL(vgl_k_mis_fill, dim3(vgl_grid(V, VGL_BLOCK, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, deg, b, L->R[0], L->R[1], L->R[2], cnt + tail0);
    }
    VGL_HIP_TRY(hipGetLastError());
    return 0;
}
// the round is done: the new tails from the mirror; a live list never grows
int mis_advance(vgl_hip_ctx *c, vgl_rc_window &w, int tail0)
{
    const int64_t was[VGL_RC_N] = {w.n(0), w.n(1), w.n(2)};
    VGL_TRY(w.advance(c->h_counters + tail0, INT64_MAX, "mis: internal error (a live list went backwards)"));      // (a ring: positions have no end)
    for (int k = 0; k < VGL_RC_N; k++)
        if (w.n(k) > was[k]) VGL_FAIL("mis: internal error (a live list grew)");
    return 0;
}

bool mis_sharded(const vgl_hip_graph *g) { return g->row_begin != 0 || g->row_end != g->V; }

}  // namespace

extern "C" {

int vgl_hip_mis_prepare(vgl_hip_ctx *c, vgl_hip_graph *g)
{
    if (!c || !g) VGL_FAIL("mis_prepare: null argument");
    if (mis_sharded(g)) VGL_FAIL("mis_prepare: graph handle must own all rows (the maximal independent set has no sharded form)");
    const vgl_simple_cache *sc = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_csr(c, g, &sc, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_mis_run(vgl_hip_ctx *c, vgl_hip_graph *g, const uint32_t *d_priority, uint32_t seed, uint8_t *d_in_set, int32_t *d_round, vgl_hip_mis_stats *stats)
{
    if (!c || !g) VGL_FAIL("mis_run: null argument");
    if (mis_sharded(g)) VGL_FAIL("mis_run: graph handle must own all rows (the maximal independent set has no sharded form)");
    if (!d_in_set && !d_round) VGL_FAIL("mis_run: all outputs are NULL (give at least one of d_in_set, d_round)");
    const vgl_simple_cache *sc = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_csr(c, g, &sc, &built));
    const vgl_simple_csr *csr = &sc->csr;
    const int32_t V = g->V;
    hipStream_t st = c->stream;
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_MIS_SHORT", "VGL_MIS_WAVE");
    vgl_hip_mis_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    if (V == 0) {
        if (stats) *stats = out;
        return 0;
    }

    // scratch of the call, all of it drawn before the loop: the state (the caller's d_round when given), the counters, the rings
    vgl_dev<int32_t> state_mem;
    vgl_dev<unsigned long long> cnt;
    if (!d_round) VGL_TRY(state_mem.alloc(st, (size_t)V));
    int32_t *state = d_round ? d_round : state_mem.p;
    VGL_TRY(cnt.alloc(st, MIS_NCNT));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * MIS_NCNT, st));
    VGL_HIP_TRY(hipMemsetAsync(state, 0, sizeof(int32_t) * (size_t)V, st));
    mis_lists L;
    VGL_TRY(mis_open_lists(c, V, csr->deg, b, cnt, MIS_TAIL, MIS_ROWS, MIS_NCNT, "mis_init", "mis_publish", &L));

    mis_graph mg;
    mg.rowptr = csr->rowptr; mg.adj = csr->adj; mg.key = mis_keys{d_priority, mis_fmix32(seed + 0x9e3779b9u)}; mg.state = state;
    const char *const slot[VGL_RC_N] = {"mis_short", "mis_wave", "mis_wg"};
    int32_t rounds = 0;
    int64_t live_total = 0;
    while (L.w.live() > 0) {
        if (rounds >= V) VGL_FAIL("mis_run: internal error (more rounds than vertices)");
        rounds++;
        live_total += L.w.live();
        VGL_TRY(vgl_rc_launch(c, slot, L.w, [&](int cls, int64_t n) {
            const unsigned long long head = (unsigned long long)L.w.head[cls];
            if (cls == VGL_RC_SHORT)
                hipLaunchKernelGGL(vgl_k_mis_short, dim3(vgl_grid(n * VGL_RC_G, VGL_BLOCK, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, L.R[cls], head, (int32_t)n, rounds, cnt.p);
            else if (cls == VGL_RC_WAVE)
                hipLaunchKernelGGL(vgl_k_mis_wave, dim3(vgl_grid(n, VGL_WAVES, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, L.R[cls], head, (int32_t)n, rounds, cnt.p);
            else
                hipLaunchKernelGGL(vgl_k_mis_wg, dim3(vgl_grid(n, 1, 4 * MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, L.R[cls], head, (int32_t)n, rounds, cnt.p);
        }));
        VGL_TRY(vgl_publish_counters(c, "mis_publish", cnt, MIS_NCNT));
        VGL_TRY(mis_advance(c, L.w, MIS_TAIL));
    }
    if (d_in_set) {
        {
            vgl_timed_launch tl(c, "mis_finish");
            hipLaunchKernelGGL(vgl_k_mis_finish, dim3(vgl_grid(V, VGL_BLOCK, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)state, d_in_set);
        }
        VGL_HIP_TRY(hipGetLastError());
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.rounds = rounds;
    out.set_size = c->h_counters[MIS_IN];
    out.live_total = live_total;
    out.entries_walked = c->h_counters[MIS_WALK];
    out.algorithmic_bytes = 12 * (int64_t)V + 24 * live_total + 8 * out.entries_walked + 8 * MIS_NCNT * (int64_t)(rounds + 1) + (d_in_set ? 5 * (int64_t)V : 0);
    if (stats) *stats = out;
    return 0;
}

int vgl_hip_matching_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int64_t *undirected_edges)
{
    if (!c || !g) VGL_FAIL("matching_prepare: null argument");
    if (mis_sharded(g)) VGL_FAIL("matching_prepare: graph handle must own all rows (the maximal matching has no sharded form)");
    const vgl_simple_cache *sg = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_edge_ids(c, g, &sg, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    if (undirected_edges) *undirected_edges = sg->ne;
    return 0;
}

int vgl_hip_matching_run(vgl_hip_ctx *c, vgl_hip_graph *g, const uint32_t *d_edge_priority, uint32_t seed, int32_t *d_edge_u, int32_t *d_edge_v, uint8_t *d_in_matching, int32_t *d_mate,
                         int32_t *d_round, vgl_hip_matching_stats *stats)
{
    if (!c || !g) VGL_FAIL("matching_run: null argument");
    if (mis_sharded(g)) VGL_FAIL("matching_run: graph handle must own all rows (the maximal matching has no sharded form)");
    if (!d_edge_u && !d_edge_v && !d_in_matching && !d_mate && !d_round)
        VGL_FAIL("matching_run: all outputs are NULL (give at least one of d_edge_u / d_edge_v, d_in_matching, d_mate, d_round)");
    if ((d_edge_u == nullptr) != (d_edge_v == nullptr)) VGL_FAIL("matching_run: d_edge_u and d_edge_v go together (both or neither)");
    const vgl_simple_cache *sg = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_edge_ids(c, g, &sg, &built));
    const vgl_simple_csr *csr = &sg->csr;
    const int32_t V = g->V;
    const int64_t ne = sg->ne;
    hipStream_t st = c->stream;
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_MIS_SHORT", "VGL_MIS_WAVE");
    vgl_hip_matching_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    out.undirected_edges = ne;
    if (V == 0) {
        if (stats) *stats = out;
        return 0;
    }
    if (d_edge_u && ne > 0) {
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_u, sg->eu, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_v, sg->ev, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
    }
    if (d_in_matching && ne > 0) VGL_HIP_TRY(hipMemsetAsync(d_in_matching, 0, (size_t)ne, st));
    if (d_round) VGL_HIP_TRY(hipMemsetAsync(d_round, 0, sizeof(int32_t) * (size_t)V, st));

    // scratch of the call, all of it drawn before the loop: mate (the caller's when given), best, the candidate list, the counters, the rings
    vgl_dev<int32_t> mate_mem, cand_mem;
    vgl_dev<unsigned long long> best, cnt;
    if (!d_mate) VGL_TRY(mate_mem.alloc(st, (size_t)V));
    int32_t *mate = d_mate ? d_mate : mate_mem.p;
    VGL_TRY(cand_mem.alloc(st, (size_t)V));
    VGL_TRY(best.alloc(st, (size_t)V));
    VGL_TRY(cnt.alloc(st, MM_NCNT));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * MM_NCNT, st));
    VGL_HIP_TRY(hipMemsetAsync(mate, 0xFF, sizeof(int32_t) * (size_t)V, st));                  // -1
    VGL_HIP_TRY(hipMemsetAsync(best, 0xFF, sizeof(unsigned long long) * (size_t)V, st));       // MM_NONE
    mis_lists L;
    VGL_TRY(mis_open_lists(c, V, csr->deg, b, cnt, MM_TAIL, MM_ROWS, MM_NCNT, "mm_init", "mm_publish", &L));

    mm_graph mg;
    mg.rowptr = csr->rowptr; mg.adj = csr->adj; mg.eid = sg->eid; mg.key = mis_keys{d_edge_priority, mis_fmix32(seed + 0x9e3779b9u)}; mg.mate = mate; mg.best = best;
    const vgl_rc_ring cand{cand_mem.p, (uint32_t)V};
    const mm_out mo{mate, d_round, d_in_matching};
    const char *const slot[VGL_RC_N] = {"mm_best_short", "mm_best_wave", "mm_best_wg"};
    int32_t rounds = 0;
    int64_t live_total = 0, cand_head = 0;
    while (L.w.live() > 0) {
        if (rounds >= V) VGL_FAIL("matching_run: internal error (more rounds than vertices)");
        rounds++;
        const int64_t live = L.w.live();
        live_total += live;
        VGL_TRY(vgl_rc_launch(c, slot, L.w, [&](int cls, int64_t n) {
            const unsigned long long head = (unsigned long long)L.w.head[cls];
            if (cls == VGL_RC_SHORT)
                hipLaunchKernelGGL(vgl_k_mm_best_short, dim3(vgl_grid(n * VGL_RC_G, VGL_BLOCK, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, L.R[cls], head, (int32_t)n, cand, cnt.p);
            else if (cls == VGL_RC_WAVE)
                hipLaunchKernelGGL(vgl_k_mm_best_wave, dim3(vgl_grid(n, VGL_WAVES, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, L.R[cls], head, (int32_t)n, cand, cnt.p);
            else
                hipLaunchKernelGGL(vgl_k_mm_best_wg, dim3(vgl_grid(n, 1, 4 * MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, mg, L.R[cls], head, (int32_t)n, cand, cnt.p);
        }));
        {
            vgl_timed_launch tl(c, "mm_match");
            hipLaunchKernelGGL(vgl_k_mm_match, dim3(vgl_grid(live, VGL_BLOCK, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, rounds, (const unsigned long long *)best.p, sg->eu, sg->ev, csr->deg, b, mo,
                               cand, (unsigned long long)cand_head, L.R[0], L.R[1], L.R[2], cnt.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(vgl_publish_counters(c, "mm_publish", cnt, MM_NCNT));
        VGL_TRY(mis_advance(c, L.w, MM_TAIL));
        const int64_t cand_tail = c->h_counters[MM_CAND];
        if (cand_tail < cand_head || cand_tail - cand_head > live) VGL_FAIL("matching_run: internal error (more candidates than live rows)");
        cand_head = cand_tail;
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.rounds = rounds;
    out.matched_edges = c->h_counters[MM_EDGES];
    out.matched_vertices = 2 * out.matched_edges;
    out.live_total = live_total;
    out.entries_walked = c->h_counters[MM_WALK];
    out.algorithmic_bytes = 20 * (int64_t)V + 28 * live_total + 12 * out.entries_walked + 8 * MM_NCNT * (int64_t)(rounds + 1) + (d_edge_u ? 16 * ne : 0) + (d_in_matching ? ne : 0) +
                            (d_round ? 4 * (int64_t)V : 0);
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
