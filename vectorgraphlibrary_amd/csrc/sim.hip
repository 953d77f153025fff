// sim.hip -- vertex similarity (common neighbours and weighted common neighbours of vertex pairs) and link prediction (the top k most similar
// vertices of a query over its 2-hop neighbourhood) on the simple undirected graph underlying the stored outgoing CSR.  The contract is written out
// in include/vgl_hip.h; DESIGN section 23 has the kernels' resources, the summation shape and the bytes models.
//
// Prepare (once per graph, cached on the handle): the symmetric CSR of vgl_simple.h (stage 1) and work2[u] = sum over v in N(u) of d(v), the number of
// 2-paths that leave u: the upper bound of a query's distinct candidates, by which the top-k rows are classified.
//
// Pairs: one counting pass validates the pairs and counts them per class of the SHORTER row (vgl_rowclass.h: short 8 lanes per pair, wave, workgroup);
// a second pass appends the pair indices to one list per class (staged appends); one kernel per class.  The lanes stride over the shorter row and
// binary-search the longer one.  Hits and weights are summed in registers in stride order, then by a fixed xor-shuffle tree (the workgroup: the four
// waves' sums added in wave order): every pair has one owner, no atomic touches an output, the weighted sum has one shape per (pair, class bounds).
//
// Top-k: one workgroup per query row, three classes by work2[u]: an LDS open-addressing table of (id, count) slots (2048 slots up to
// VGL_SIM_TABLE_SMALL, 16384 up to VGL_SIM_TABLE), or a dense int32 counter array of V entries and a touched list in a scratch slot of the workgroup
// (beyond).  The row is expanded by walking N(v) for every v in N(u); u itself and, unless asked otherwise, N(u) are struck out afterwards; then k
// rounds of a workgroup arg-max over the candidates that come strictly after the previous pick in the total order (score as an int64 fraction
// comparison, ties to the smaller label).  The touched list clears the counters for the slot's next row.
#include "vgl_simple.h"
#include "vgl_rowclass.h"
#include <cstring>
#include <algorithm>
#include <vector>

namespace {

constexpr int64_t SIM_MAX_GRID = 2048;           // workgroups of a grid-stride kernel
constexpr int SIM_SLOTS_S = 2048, SIM_SLOTS_L = 16384;      // (id, count) slots of the two table classes: 16 KiB and 128 KiB of LDS
constexpr int SIM_TG = 16;                       // lanes that stream one N(v) in the table kernels (the global kernel: a wavefront)
constexpr int64_t SIM_MAX_SLOTS = 1024;          // scratch slots (resident workgroups) of the global class at most
enum { SIM_SMALL = 0, SIM_TABLE = 1, SIM_GLOBAL = 2 };
enum {
    SIM_TAIL = 0,       // + class: items appended to the class list so far
    SIM_ROWS = 3,       // + class: items per class
    SIM_BAD = 6,        // vertices outside [0, V)
    SIM_WORK = 7,       // pairs: sum of min(d(u), d(v)); top-k: sum of work2 over the queries
    SIM_COMMON = 8,     // pairs: sum of c
    SIM_CAND = 9,       // top-k: distinct candidates after the exclusion
    SIM_FILLED = 10,    // top-k: output slots that hold a vertex
    SIM_BADW = 11,      // weights that are NaN, infinite or negative
    SIM_NCNT = 12
};
static_assert(SIM_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

// ---- prepare: work2[u] = sum of d(v) over v in N(u), 8 lanes per row ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sim_work2(int32_t V, const int64_t *rowptr, const int32_t *adj, const int32_t *deg, int64_t *work2)
{
    const int gi = threadIdx.x & (VGL_RC_G - 1);
    for (int64_t base = (int64_t)blockIdx.x * (VGL_BLOCK / VGL_RC_G); base < V; base += (int64_t)gridDim.x * (VGL_BLOCK / VGL_RC_G)) {      // (uniform over the workgroup)
        const int64_t u = base + threadIdx.x / VGL_RC_G;
        int64_t s = 0;
        if (u < V)
            for (int64_t e = rowptr[u] + gi; e < rowptr[u + 1]; e += VGL_RC_G) s += deg[adj[e]];
#pragma unroll
        for (int o = VGL_RC_G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (gi == 0 && u < V) work2[u] = s;
    }
}
// weights that are not finite values >= 0 (a NaN fails every comparison)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sim_check_weights(int32_t V, const double *weight, unsigned long long *bad)
{
    int64_t n = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK)
        if (!(weight[v] >= 0.0 && weight[v] <= 1.7976931348623157e308)) n++;
    vgl_wave_flush_add(bad, n);
}

// ---- the class lists (vgl_rc_lists): cls(i, work) = the class of item i and its work, or -1 for a vertex out of range ----
struct sim_pair_src {
    const int32_t *u, *v;
    int32_t V;
    const int32_t *deg;
    vgl_rc_bounds b;
    __device__ __forceinline__ int cls(int64_t i, int64_t &work) const
    {
        const int32_t x = u[i], y = v[i];
        if (x < 0 || x >= V || y < 0 || y >= V) return -1;
        work = min(deg[x], deg[y]);
        return vgl_rc_class_of(work, b);
    }
};
struct sim_query_src {
    const int32_t *q;            // nullptr: item i asks for vertex i
    int32_t V;
    const int64_t *work2;
    int64_t small, table;
    __device__ __forceinline__ int cls(int64_t i, int64_t &work) const
    {
        const int32_t x = q ? q[i] : (int32_t)i;
        if (x < 0 || x >= V) return -1;
        work = work2[x];
        return work <= small ? SIM_SMALL : work <= table ? SIM_TABLE : SIM_GLOBAL;
    }
};

// ---- pairs ----
struct sim_pairs_args {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    const int32_t *u, *v;        // the pairs of this chunk
    const double *weight;
    int32_t *common;             // of this chunk, or nullptr
    double *weighted;            // of this chunk, or nullptr
    unsigned long long *cnt;
};
// the rows of pair p: the shorter one (ss, sn) and the longer one (ls, ln); u's row is the shorter one when they are equally long
struct sim_rows { int64_t ss, ls; int sn, ln; };
__device__ __forceinline__ sim_rows sim_rows_of(const sim_pairs_args &a, int64_t p)
{
    const int32_t u = a.u[p], v = a.v[p];
    const int64_t su = a.rowptr[u], sv = a.rowptr[v];
    const int du = (int)(a.rowptr[u + 1] - su), dv = (int)(a.rowptr[v + 1] - sv);
    return du <= dv ? sim_rows{su, sv, du, dv} : sim_rows{sv, su, dv, du};
}
// entries first, first + stride, ... of the shorter row, in that order: the hits and (W) the sum of their weights
template <bool W>
__device__ __forceinline__ void sim_walk(const sim_pairs_args &a, const sim_rows &r, int first, int stride, int &hits, double &sum)
{
    for (int i = first; i < r.sn; i += stride) {
        const int32_t x = a.adj[r.ss + i];
        if (vgl_contains(a.adj, r.ls, r.ln, x)) {
            hits++;
            if (W) sum += a.weight[x];
        }
    }
}
template <int CLS, bool W>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sim_pairs(const int32_t *list, int32_t n, sim_pairs_args a)
{
    using T = vgl_rc_team<CLS>;
    int64_t total = 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int64_t p = 0;
        sim_rows r{0, 0, 0, 0};
        if (has) {
            p = list[i];
            r = sim_rows_of(a, p);
        }
        int hits = 0;
        double sum = 0.0;
        sim_walk<W>(a, r, T::lane(), T::LANES, hits, sum);
        hits = T::sum_of(hits);
        if (W) sum = T::sum_of(sum);                                  // (the workgroup: the waves' sums, added in wave order)
        if (T::lead() && has) {
            total += hits;
            if (a.common) a.common[p] = hits;
            if (W) a.weighted[p] = sum;
        }
    }
    vgl_wave_flush_add(a.cnt + SIM_COMMON, total);
}

// ---- top-k ----
struct sim_topk_args {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    const int32_t *deg;
    const int64_t *work2;
    const int32_t *queries;      // nullptr: row i asks for vertex i
    const int32_t *label;        // nullptr: the vertex id
    int32_t *ids, *common;       // n x k; common may be nullptr
    int metric, k, include;
    unsigned long long *cnt;
};
// a candidate under the total order: the score num / den (den >= 1), then the smaller label; id < 0: none (after every candidate)
struct sim_cand { int32_t num, den, label, id; };
__device__ __forceinline__ bool sim_before(const sim_cand &x, const sim_cand &y)
{
    if (x.id < 0) return false;
    if (y.id < 0) return true;
    const int64_t l = (int64_t)x.num * y.den, r = (int64_t)y.num * x.den;
    return l > r || (l == r && x.label < y.label);
}
__device__ __forceinline__ sim_cand sim_cand_of(const sim_topk_args &a, int32_t du, int32_t w, int32_t c)
{
    const int32_t dw = a.deg[w];
    const int32_t den = a.metric == VGL_HIP_SIM_COMMON ? 1 : a.metric == VGL_HIP_SIM_JACCARD ? du + dw - c : min(du, dw);
    return sim_cand{c, den, a.label ? a.label[w] : w, w};
}

// where the counted candidates of a row live: entry i of n is the vertex w with c common neighbours (c <= 0: no candidate)
struct sim_table_src {
    const int32_t *id, *count;
    int n;
    __device__ __forceinline__ void get(int i, int32_t &w, int32_t &c) const
    {
        w = id[i];
        c = w >= 0 ? count[i] : 0;
    }
};
struct sim_global_src {
    const int32_t *touched, *counter;
    int n;
    __device__ __forceinline__ void get(int i, int32_t &w, int32_t &c) const
    {
        w = touched[i];
        c = vgl_load_agent(counter + w);
    }
};
// Row `row` of the output (query u): k rounds of a workgroup arg-max over the candidates that come strictly after the previous pick; the rest of
// the row is padded.  Every thread of the workgroup calls; cand / filled are the thread's running sums for the kernel's counters.
template <class SRC>
__device__ __forceinline__ void sim_select(const sim_topk_args &a, int64_t row, int32_t u, const SRC &src, sim_cand *s_best, int64_t &cand, int64_t &filled)
{
    const int32_t du = a.deg[u];
    int32_t *ids = a.ids + row * a.k;
    int32_t *common = a.common ? a.common + row * a.k : nullptr;
    sim_cand prev{0, 1, 0, -1};
    int r = 0;
    for (; r < a.k; r++) {                                            // (uniform over the workgroup)
        sim_cand best{0, 1, 0, -1};
        for (int i = threadIdx.x; i < src.n; i += VGL_BLOCK) {
            int32_t w, c;
            src.get(i, w, c);
            if (c <= 0) continue;
            if (r == 0) cand++;
            const sim_cand x = sim_cand_of(a, du, w, c);
            if (r > 0 && !sim_before(prev, x)) continue;
            if (sim_before(x, best)) best = x;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const sim_cand y{__shfl_xor(best.num, o), __shfl_xor(best.den, o), __shfl_xor(best.label, o), __shfl_xor(best.id, o)};
            if (sim_before(y, best)) best = y;
        }
        __syncthreads();                                              // the picks of the round before have been read
        if (vgl_lane() == 0) s_best[vgl_wave()] = best;
        __syncthreads();
        best = s_best[0];
#pragma unroll
        for (int w = 1; w < VGL_WAVES; w++)
            if (sim_before(s_best[w], best)) best = s_best[w];
        if (best.id < 0) break;                                       // (uniform: every thread holds the same pick)
        if (threadIdx.x == 0) {
            ids[r] = best.id;
            if (common) common[r] = best.num;
        }
        prev = best;
    }
    if (threadIdx.x == 0) filled += r;
    for (int j = r + threadIdx.x; j < a.k; j += VGL_BLOCK) {
        ids[j] = -1;
        if (common) common[j] = 0;
    }
}

template <int SLOTS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sim_topk_table(sim_topk_args a, const int32_t *list, int32_t n)
{
    __shared__ int32_t s_id[SLOTS];
    __shared__ int32_t s_cnt[SLOTS];
    __shared__ sim_cand s_best[VGL_WAVES];
    const int gi = threadIdx.x & (SIM_TG - 1);
    int64_t cand = 0, filled = 0;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {             // (uniform over the workgroup)
        const int64_t row = list[i];
        const int32_t u = a.queries ? a.queries[row] : (int32_t)row;
        const int64_t su = a.rowptr[u], du = a.rowptr[u + 1] - su;
        const int64_t w2 = a.work2[u];                                // at least the distinct candidates; <= SLOTS / 2 by the class
        int bits = 6;
        while ((1 << bits) < 2 * w2 && (1 << bits) < SLOTS) bits++;
        const uint32_t mask = (1u << bits) - 1u;
        __syncthreads();                                              // the table of the row before has been read
        for (int j = threadIdx.x; j <= (int)mask; j += VGL_BLOCK) { s_id[j] = -1; s_cnt[j] = 0; }
        __syncthreads();
        for (int64_t j = threadIdx.x / SIM_TG; j < du; j += VGL_BLOCK / SIM_TG) {
            const int32_t v = a.adj[su + j];
            const int64_t sv = a.rowptr[v], dv = a.rowptr[v + 1] - sv;
            for (int64_t p = gi; p < dv; p += SIM_TG) {
                const int32_t w = a.adj[sv + p];
                uint32_t h = vgl_hash(w, bits);
                for (uint32_t t = 0; t <= mask; t++) {                // (the table is at most half full: a free slot comes long before the bound)
                    const int32_t old = atomicCAS(&s_id[h], -1, w);
                    if (old == -1 || old == w) { atomicAdd(&s_cnt[h], 1); break; }
                    h = (h + 1) & mask;
                }
            }
        }
        __syncthreads();
        // struck out: u itself (a 2-path u - v - u per neighbour) and, for link prediction, the neighbours
        for (int64_t j = (int64_t)threadIdx.x - 1; j < (a.include ? 0 : du); j += VGL_BLOCK) {
            const int32_t w = j < 0 ? u : a.adj[su + j];
            uint32_t h = vgl_hash(w, bits);
            for (uint32_t t = 0; t <= mask; t++) {
                const int32_t x = s_id[h];
                if (x == -1) break;
                if (x == w) { s_cnt[h] = 0; break; }
                h = (h + 1) & mask;
            }
        }
        __syncthreads();
        sim_select(a, row, u, sim_table_src{s_id, s_cnt, (int)mask + 1}, s_best, cand, filled);
    }
    vgl_wave_flush_add(a.cnt + SIM_CAND, cand);
    vgl_wave_flush_add(a.cnt + SIM_FILLED, filled);
}

// workgroup b owns scratch slot b: V counters (all 0 between rows) and a touched list of V entries
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sim_topk_global(sim_topk_args a, const int32_t *list, int32_t n, int32_t V, int32_t *scratch)
{
    __shared__ int s_touched;
    __shared__ sim_cand s_best[VGL_WAVES];
    int32_t *counter = scratch + (int64_t)blockIdx.x * 2 * V;
    int32_t *touched = counter + V;
    const int lane = vgl_lane();
    int64_t cand = 0, filled = 0;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {             // (uniform over the workgroup)
        const int64_t row = list[i];
        const int32_t u = a.queries ? a.queries[row] : (int32_t)row;
        const int64_t su = a.rowptr[u], du = a.rowptr[u + 1] - su;
        __syncthreads();                                              // the list of the row before has been read
        if (threadIdx.x == 0) s_touched = 0;
        __syncthreads();
        for (int64_t j = vgl_wave(); j < du; j += VGL_WAVES) {        // a wavefront per neighbour's row
            const int32_t v = a.adj[su + j];
            const int64_t sv = a.rowptr[v], dv = a.rowptr[v + 1] - sv;
            for (int64_t p = lane; p < dv; p += 64) {
                const int32_t w = a.adj[sv + p];
                if (atomicAdd(counter + w, 1) == 0) {                 // the first 2-path to w: at most V of them, the list cannot overflow
                    const int at = atomicAdd(&s_touched, 1);
                    if (at < V) touched[at] = w;
                }
            }
        }
        __syncthreads();
        for (int64_t j = (int64_t)threadIdx.x - 1; j < (a.include ? 0 : du); j += VGL_BLOCK) vgl_store_agent(counter + (j < 0 ? u : a.adj[su + j]), 0);
        __syncthreads();
        const int nt = min(s_touched, V);
        sim_select(a, row, u, sim_global_src{touched, counter, nt}, s_best, cand, filled);
        __syncthreads();
        for (int j = threadIdx.x; j < nt; j += VGL_BLOCK) vgl_store_agent(counter + touched[j], 0);
    }
    vgl_wave_flush_add(a.cnt + SIM_CAND, cand);
    vgl_wave_flush_add(a.cnt + SIM_FILLED, filled);
}

bool sim_sharded(const vgl_hip_graph *g) { return g->row_begin != 0 || g->row_end != g->V; }

}  // namespace

// What the handle keeps for the similarity entries besides the symmetric CSR (freed with the handle)
struct vgl_sim_cache {
    vgl_dev<int64_t> work2;                      // V: the 2-paths that leave every vertex
};
template <> void vgl_cache_free(vgl_sim_cache *p) { delete p; }

namespace {

// the symmetric CSR and work2; *built: this call built work2
int sim_ensure(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_simple_cache **sc, const vgl_sim_cache **out, bool *built)
{
    bool csr_built = false;
    VGL_TRY(vgl_simple_ensure_csr(c, g, sc, &csr_built));
    *built = false;
    if (!g->sim) {
        vgl_cache<vgl_sim_cache> p(new vgl_sim_cache());
        VGL_TRY(p->work2.alloc((size_t)g->V));
        const vgl_simple_csr &csr = (*sc)->csr;
        {
            vgl_timed_launch tl(c, "sim_work2");
            hipLaunchKernelGGL(vgl_k_sim_work2, dim3(vgl_grid((int64_t)g->V * VGL_RC_G, VGL_BLOCK, SIM_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream, g->V, (const int64_t *)csr.rowptr.p,
                               (const int32_t *)csr.adj.p, (const int32_t *)csr.deg.p, p->work2.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_HIP_TRY(hipStreamSynchronize(c->stream));
        g->sim = std::move(p);
        *built = true;
    }
    *out = g->sim.get();
    return 0;
}

const int64_t sim_pairs_cap[VGL_RC_N] = {4 * SIM_MAX_GRID, 4 * SIM_MAX_GRID, 4 * SIM_MAX_GRID};
const char *const sim_pairs_slot[VGL_RC_N] = {"sim_pairs_short", "sim_pairs_wave", "sim_pairs_wg"};

}  // namespace

extern "C" {

int vgl_hip_sim_prepare(vgl_hip_ctx *c, vgl_hip_graph *g)
{
    if (!c || !g) VGL_FAIL("sim_prepare: null argument");
    if (sim_sharded(g)) VGL_FAIL("sim_prepare: graph handle must own all rows (vertex similarity has no sharded form)");
    const vgl_simple_cache *sc = nullptr;
    const vgl_sim_cache *sm = nullptr;
    bool built = false;
    VGL_TRY(sim_ensure(c, g, &sc, &sm, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_sim_pairs(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *d_u, const int32_t *d_v, int64_t n, const double *d_weight, int32_t *d_common, double *d_weighted, int32_t *d_degree,
                      vgl_hip_sim_pairs_stats *stats)
{
    if (!c || !g) VGL_FAIL("sim_pairs: null argument");
    if (sim_sharded(g)) VGL_FAIL("sim_pairs: graph handle must own all rows (vertex similarity has no sharded form)");
    if (n < 0) VGL_FAIL("sim_pairs: n is negative");
    if (n > 0 && (!d_u || !d_v)) VGL_FAIL("sim_pairs: d_u and d_v must not be NULL");
    if (!d_common && !d_weighted) VGL_FAIL("sim_pairs: all outputs are NULL (give at least one of d_common, d_weighted)");
    if (d_weighted && !d_weight) VGL_FAIL("sim_pairs: d_weighted needs d_weight");
    const vgl_simple_cache *sc = nullptr;
    const vgl_sim_cache *sm = nullptr;
    bool built = false;
    VGL_TRY(sim_ensure(c, g, &sc, &sm, &built));
    const vgl_simple_csr *csr = &sc->csr;
    const int32_t V = g->V;
    hipStream_t st = c->stream;
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_SIM_SHORT", "VGL_SIM_WAVE");
    const int64_t chunk = vgl_env_int(c, "VGL_SIM_PAIR_CHUNK", (int64_t)1 << 28, 1024, (int64_t)1 << 30);      // pairs per list build: the list entries are int32
    vgl_hip_sim_pairs_stats out;
    memset(&out, 0, sizeof(out));
    out.pairs = n;
    out.prepared_now = built ? 1 : 0;

    vgl_dev<unsigned long long> cnt;
    VGL_TRY(vgl_open_counters(c, &cnt, SIM_NCNT));
    // pass 1, nothing written yet: the weights, then every chunk of pairs validated and counted per class
    if (d_weighted && V > 0) {
        {
            vgl_timed_launch tl(c, "sim_classify");
            hipLaunchKernelGGL(vgl_k_sim_check_weights, dim3(vgl_grid(V, VGL_BLOCK, SIM_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, d_weight, cnt + SIM_BADW);
        }
        VGL_HIP_TRY(hipGetLastError());
    }
    std::vector<int64_t> rows;                                        // VGL_RC_N per chunk
    for (int64_t base = 0; base < n; base += chunk) {
        const int64_t m = std::min(chunk, n - base);
        const sim_pair_src src{d_u + base, d_v + base, V, csr->deg, b};
        vgl_rc_lists<vgl_rc_bounded> L;
        VGL_TRY(L.count(c, "sim_classify", "sim_publish", src, m, SIM_MAX_GRID, cnt.p, SIM_NCNT, SIM_ROWS, SIM_BAD, SIM_WORK, m, "sim_pairs: a vertex of a pair is outside [0, V)",
                        "sim_pairs: internal error (the classes do not add up to the pairs)"));
        rows.insert(rows.end(), L.rows, L.rows + VGL_RC_N);
        VGL_HIP_TRY(hipMemsetAsync(cnt + SIM_ROWS, 0, sizeof(unsigned long long) * VGL_RC_N, st));
    }
    if (n == 0) VGL_TRY(vgl_publish_counters(c, "sim_publish", cnt, SIM_NCNT));
    if (c->h_counters[SIM_BADW] != 0) VGL_FAIL("sim_pairs: a weight is NaN, infinite or negative");
    out.elements_examined = c->h_counters[SIM_WORK];

    // pass 2: the lists of a chunk, one kernel per class
    if (d_degree && V > 0) VGL_HIP_TRY(hipMemcpyAsync(d_degree, csr->deg, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToDevice, st));
    vgl_dev<int32_t> list;
    if (n > 0) VGL_TRY(list.alloc(st, (size_t)std::min(chunk, n)));
    for (int64_t base = 0, at = 0; base < n; base += chunk, at += VGL_RC_N) {
        const int64_t m = std::min(chunk, n - base);
        const sim_pair_src src{d_u + base, d_v + base, V, csr->deg, b};
        vgl_rc_lists<vgl_rc_bounded> L;
        std::copy(&rows[(size_t)at], &rows[(size_t)at] + VGL_RC_N, L.rows);
        VGL_HIP_TRY(hipMemsetAsync(cnt + SIM_TAIL, 0, sizeof(unsigned long long) * VGL_RC_N, st));
        VGL_TRY(L.fill(c, "sim_classify", src, m, SIM_MAX_GRID, 1, list.p, cnt + SIM_TAIL));
        const int32_t *const of[VGL_RC_N] = {L.l[0].rows, L.l[1].rows, L.l[2].rows};
        const sim_pairs_args a{csr->rowptr, csr->adj, d_u + base, d_v + base, d_weight, d_common ? d_common + base : nullptr, d_weighted ? d_weighted + base : nullptr, cnt.p};
        if (d_weighted)
            VGL_TRY(vgl_rc_launch_trio(c, sim_pairs_slot, L.rows, sim_pairs_cap, vgl_k_sim_pairs<VGL_RC_SHORT, true>, vgl_k_sim_pairs<VGL_RC_WAVE, true>, vgl_k_sim_pairs<VGL_RC_WG, true>, of, a));
        else
            VGL_TRY(vgl_rc_launch_trio(c, sim_pairs_slot, L.rows, sim_pairs_cap, vgl_k_sim_pairs<VGL_RC_SHORT, false>, vgl_k_sim_pairs<VGL_RC_WAVE, false>, vgl_k_sim_pairs<VGL_RC_WG, false>, of, a));
        out.pairs_short += rows[(size_t)at + VGL_RC_SHORT];
        out.pairs_wave += rows[(size_t)at + VGL_RC_WAVE];
        out.pairs_wg += rows[(size_t)at + VGL_RC_WG];
    }
    if (n > 0) VGL_TRY(vgl_publish_counters(c, "sim_publish", cnt, SIM_NCNT));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.common_total = c->h_counters[SIM_COMMON];
    out.algorithmic_bytes = 64 * n + 4 * out.elements_examined + (d_common ? 4 * n : 0) + (d_weighted ? 8 * n + 8 * out.common_total + 8 * (int64_t)V : 0) + (d_degree ? 8 * (int64_t)V : 0);
    if (stats) *stats = out;
    return 0;
}

int vgl_hip_sim_topk(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *d_queries, int32_t n, int metric, int32_t k, int include_neighbours, const int32_t *d_label, int32_t *d_ids,
                     int32_t *d_common, vgl_hip_sim_topk_stats *stats)
{
    if (!c || !g) VGL_FAIL("sim_topk: null argument");
    if (sim_sharded(g)) VGL_FAIL("sim_topk: graph handle must own all rows (vertex similarity has no sharded form)");
    if (k < 1 || k > VGL_HIP_SIM_MAX_K) VGL_FAIL("sim_topk: k must be in [1, VGL_HIP_SIM_MAX_K]");
    if (metric != VGL_HIP_SIM_COMMON && metric != VGL_HIP_SIM_JACCARD && metric != VGL_HIP_SIM_OVERLAP) VGL_FAIL("sim_topk: unknown metric");
    if (n < 0) VGL_FAIL("sim_topk: n is negative");
    if (!d_queries && n != g->V) VGL_FAIL("sim_topk: without d_queries every vertex is a query: n must equal V");
    if (!d_ids) VGL_FAIL("sim_topk: d_ids must not be NULL");
    const vgl_simple_cache *sc = nullptr;
    const vgl_sim_cache *sm = nullptr;
    bool built = false;
    VGL_TRY(sim_ensure(c, g, &sc, &sm, &built));
    const vgl_simple_csr *csr = &sc->csr;
    const int32_t V = g->V;
    hipStream_t st = c->stream;
    const int64_t small = vgl_env_int(c, "VGL_SIM_TABLE_SMALL", SIM_SLOTS_S / 2, 0, SIM_SLOTS_S / 2);
    const int64_t table = vgl_env_int(c, "VGL_SIM_TABLE", SIM_SLOTS_L / 2, small, SIM_SLOTS_L / 2);
    const int64_t scratch_mb = vgl_env_int(c, "VGL_SIM_SCRATCH_MB", 4096, 1, 1 << 20);
    vgl_hip_sim_topk_stats out;
    memset(&out, 0, sizeof(out));
    out.queries = n;
    out.prepared_now = built ? 1 : 0;
    if (n == 0) {
        if (stats) *stats = out;
        return 0;
    }

    vgl_dev<unsigned long long> cnt;
    VGL_TRY(vgl_open_counters(c, &cnt, SIM_NCNT));
    const sim_query_src src{d_queries, V, sm->work2, small, table};
    vgl_rc_lists<vgl_rc_bounded> L;
    VGL_TRY(L.count(c, "sim_classify", "sim_publish", src, (int64_t)n, SIM_MAX_GRID, cnt.p, SIM_NCNT, SIM_ROWS, SIM_BAD, SIM_WORK, n, "sim_topk: a query is outside [0, V)",
                    "sim_topk: internal error (the classes do not add up to the queries)"));
    const int64_t *rows = L.rows;
    out.rows_small = rows[SIM_SMALL];
    out.rows_table = rows[SIM_TABLE];
    out.rows_global = rows[SIM_GLOBAL];
    out.two_paths_walked = c->h_counters[SIM_WORK];

    vgl_dev<int32_t> scratch;
    VGL_TRY(L.fill(c, "sim_classify", src, (int64_t)n, SIM_MAX_GRID, 1, nullptr, cnt + SIM_TAIL));
    int64_t slots = 0;
    if (rows[SIM_GLOBAL] > 0) {                                       // a slot: V counters and V list entries; as many as the budget holds, at least 1
        slots = std::max<int64_t>(1, std::min((scratch_mb << 20) / (8 * (int64_t)V), std::min(rows[SIM_GLOBAL], SIM_MAX_SLOTS)));
        VGL_TRY(scratch.alloc(st, (size_t)(slots * 2 * V)));
        VGL_HIP_TRY(hipMemsetAsync(scratch.p, 0, sizeof(int32_t) * (size_t)(slots * 2 * V), st));
    }
    out.scratch_slots = slots;
    const sim_topk_args a{csr->rowptr, csr->adj, csr->deg, sm->work2, d_queries, d_label, d_ids, d_common, metric, k, include_neighbours ? 1 : 0, cnt.p};
    const char *const slot[VGL_RC_N] = {"sim_topk_small", "sim_topk_table", "sim_topk_global"};
    VGL_TRY(vgl_rc_launch(c, slot, rows, [&](int cls, int64_t m) {
        const int32_t *l = L.l[cls].rows;
        if (cls == SIM_SMALL)
            hipLaunchKernelGGL(vgl_k_sim_topk_table<SIM_SLOTS_S>, dim3(vgl_grid(m, 1, 4 * SIM_MAX_GRID)), dim3(VGL_BLOCK), 0, st, a, l, (int32_t)m);
        else if (cls == SIM_TABLE)
            hipLaunchKernelGGL(vgl_k_sim_topk_table<SIM_SLOTS_L>, dim3(vgl_grid(m, 1, SIM_MAX_GRID)), dim3(VGL_BLOCK), 0, st, a, l, (int32_t)m);
        else
            hipLaunchKernelGGL(vgl_k_sim_topk_global, dim3((unsigned)slots), dim3(VGL_BLOCK), 0, st, a, l, (int32_t)m, V, scratch.p);
    }));
    VGL_TRY(vgl_publish_counters(c, "sim_publish", cnt, SIM_NCNT));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.candidates_total = c->h_counters[SIM_CAND];
    out.filled = c->h_counters[SIM_FILLED];
    out.algorithmic_bytes = 36 * (int64_t)n + 4 * out.two_paths_walked + (d_common ? 8 : 4) * (int64_t)n * k;
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
