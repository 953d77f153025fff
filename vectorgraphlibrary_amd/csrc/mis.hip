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

// key(i, seed) = fmix32(i ^ mix), mix = fmix32(seed + 0x9e3779b9); or the caller's array
struct mis_keys {
    const uint32_t *prio; uint32_t mix;
    __device__ __forceinline__ uint32_t of(int32_t i) const { return prio ? prio[i] : vgl_fmix32((uint32_t)i ^ mix); }
};

// ---- the live lists: every vertex, by the length of its row ----
struct mis_row_src {
    const int32_t *deg; vgl_rc_bounds b;
    __device__ __forceinline__ int cls(int64_t v, int64_t &) const { return vgl_rc_class_of(deg[v], b); }
};
// the live rows of a class in a round: positions head, head + 1, ... of its ring
struct mis_live {
    vgl_rc_ring R; unsigned long long head;
    __device__ __forceinline__ int32_t at(int64_t i) const { return R.rows[(head + (unsigned long long)i) % R.cap]; }
};

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
// a team per row; the wave's scan stops at the first earlier neighbour that is IN
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mis(mis_live l, int32_t n, mis_graph g, int32_t r, unsigned long long *cnt)
{
    using T = vgl_rc_team<CLS>;
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    int64_t walked = 0, in = 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int32_t v = 0;
        uint32_t kv = 0;
        int64_t lo = 0, hi = 0;
        if (has) {
            v = l.at(i);
            kv = g.key.of(v);
            lo = g.rowptr[v]; hi = g.rowptr[v + 1];
        }
        int bits = 0;
        if constexpr (CLS == VGL_RC_WAVE) {
            for (int64_t e = lo; e < hi; e += T::LANES) {             // (uniform over the wave)
                if (e + T::lane() < hi) bits |= mis_look(g, v, kv, g.adj[e + T::lane()], r);
                if (__any(bits & 1)) break;
            }
        } else
            for (int64_t e = lo + T::lane(); e < hi; e += T::LANES) bits |= mis_look(g, v, kv, g.adj[e], r);
        bits = T::or_of(bits, 2);
        bool again = false;
        if (T::lead() && has) {
            walked += hi - lo;
            again = mis_decide(g, v, bits, r, in);
        }
        st[0].keep(again, v, l.R, cnt + MIS_TAIL + CLS);
    }
    st[0].flush(l.R, cnt + MIS_TAIL + CLS);
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
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_mm_best(mis_live l, int32_t n, mm_graph g, vgl_rc_ring cand, unsigned long long *cnt)
{
    using T = vgl_rc_team<CLS>;
    vgl_rc_stage st[1];
    vgl_rc_stage_open(st);
    int64_t walked = 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n, lead = T::lead() && has;
        int32_t v = 0;
        int64_t lo = 0, hi = 0;
        if (has) {
            v = l.at(i);
            lo = g.rowptr[v]; hi = g.rowptr[v + 1];
        }
        const unsigned long long m = T::min_of(mm_walk(lo + T::lane(), hi, T::LANES, g));
        if (lead) {
            walked += hi - lo;
            g.best[v] = m;
        }
        st[0].keep(lead && m != MM_NONE, v, cand, cnt + MM_CAND);
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
    vgl_rc_lists<vgl_rc_ring> L;
    vgl_rc_window w;
    // the live rows of the round, per class
    void live(mis_live (&l)[VGL_RC_N]) const
    {
        for (int k = 0; k < VGL_RC_N; k++) l[k] = mis_live{L.l[k], (unsigned long long)w.head[k]};
    }
};
const int64_t mis_grid_cap[VGL_RC_N] = {MIS_MAX_GRID, MIS_MAX_GRID, 4 * MIS_MAX_GRID};      // workgroups of a class's launch at most
// every vertex into the ring of its class (cnt + tail0: the three tails; cnt + rows0: the three row counts); one host read
int mis_open_lists(vgl_hip_ctx *c, int32_t V, const int32_t *deg, vgl_rc_bounds b, unsigned long long *cnt, int tail0, int rows0, int ncnt, const char *slot_init, const char *slot_publish,
                   mis_lists *M)
{
    const mis_row_src src{deg, b};
    VGL_TRY(M->L.count(c, slot_init, slot_publish, src, V, MIS_MAX_GRID, cnt, ncnt, rows0, -1, -1, -1, nullptr, "mis: internal error (the classes do not add up to the vertices)"));
    for (int k = 0; k < VGL_RC_N; k++)
        if (M->L.rows[k] > V) VGL_FAIL("mis: internal error (more rows in a class than vertices)");
    if (M->L.rows[0] + M->L.rows[1] + M->L.rows[2] != V) VGL_FAIL("mis: internal error (the classes do not add up to the vertices)");
    VGL_TRY(M->L.fill(c, slot_init, src, V, MIS_MAX_GRID, 2, nullptr, cnt + tail0));
    for (int k = 0; k < VGL_RC_N; k++) M->w.tail[k] = M->L.rows[k];
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
    mg.rowptr = csr->rowptr; mg.adj = csr->adj; mg.key = mis_keys{d_priority, vgl_fmix32(seed + 0x9e3779b9u)}; mg.state = state;
    const char *const slot[VGL_RC_N] = {"mis_short", "mis_wave", "mis_wg"};
    int32_t rounds = 0;
    int64_t live_total = 0;
    while (L.w.live() > 0) {
        if (rounds >= V) VGL_FAIL("mis_run: internal error (more rounds than vertices)");
        rounds++;
        live_total += L.w.live();
        mis_live rows[VGL_RC_N];
        L.live(rows);
        VGL_TRY(vgl_rc_launch_trio(c, slot, L.w, mis_grid_cap, vgl_k_mis<VGL_RC_SHORT>, vgl_k_mis<VGL_RC_WAVE>, vgl_k_mis<VGL_RC_WG>, rows, mg, rounds, cnt.p));
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
    mg.rowptr = csr->rowptr; mg.adj = csr->adj; mg.eid = sg->eid; mg.key = mis_keys{d_edge_priority, vgl_fmix32(seed + 0x9e3779b9u)}; mg.mate = mate; mg.best = best;
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
        mis_live rows[VGL_RC_N];
        L.live(rows);
        VGL_TRY(vgl_rc_launch_trio(c, slot, L.w, mis_grid_cap, vgl_k_mm_best<VGL_RC_SHORT>, vgl_k_mm_best<VGL_RC_WAVE>, vgl_k_mm_best<VGL_RC_WG>, rows, mg, cand, cnt.p));
        {
            vgl_timed_launch tl(c, "mm_match");
            hipLaunchKernelGGL(vgl_k_mm_match, dim3(vgl_grid(live, VGL_BLOCK, MIS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, rounds, (const unsigned long long *)best.p, sg->eu, sg->ev, csr->deg, b, mo,
                               cand, (unsigned long long)cand_head, L.L.l[0], L.L.l[1], L.L.l[2], cnt.p);
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
