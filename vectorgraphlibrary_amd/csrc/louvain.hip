// louvain.hip -- one Louvain level by synchronous integer move rounds: every round evaluates all vertices against one snapshot of the assignment,
// half of the vertices (a hash of id and round) may move, the exact modularity numerator N = m I - sum tot^2 judges the round before.  A level ends
// converged, reverted, with a small gain or at its round cap.  The contract is written out in include/vgl_hip.h; DESIGN section 27 has the kernels,
// their bounds and the bytes model.  The multi-level run (quotient levels in between) is not here: see DESIGN section 27.
//
// Evaluate: rows are classified once per level by length (vgl_rowclass.h bounds plus a fourth, sorted class) and listed per class.
//   short   8 lanes per row: rank-counting among the gathered comm[adj], a chunk of 8 in registers at a time, shuffles within the team; an entry is a
//           head when no equal key sits earlier, k(v, C) at a head is the sum over the equal keys
//   wave    a wavefront per row, wg: a workgroup per row: keys staged in LDS, a bitonic sort, an in-place compaction of the distinct keys with the
//           team's rank, one LDS int64 sum per distinct key (binary search, LDS integer add); 12 bytes per entry
//   sorted  64-bit keys  row << 32 | comm[w]  paired with the weight (a self entry's key sorts behind every id): a radix sort of pairs + a reduce by
//           key (vgl_prim.h) in pieces of consecutive rows under VGL_LOUVAIN_SORT_CAP_MB, then a wavefront per row scores the row's runs
// Every class ends in the same pick: the greatest score, then the smallest id among the equal scores, then the own community and the swap guard.
// No floating point, no cooperative launch, no wait on a flag, no retry loop: integer sums and integer atomics only.
#include "vgl_rowclass.h"
#include "vgl_prim.h"
#include <cstring>
#include <algorithm>
#include <vector>

namespace {
constexpr int LV_WAVE_CAP = 1024;                // LDS keys and sums per wavefront row
constexpr int LV_WG_CAP = 4096;                  // ... per workgroup row: 4096 x (4 + 8) bytes = 48 KiB, the same as four wavefront rows
constexpr int LV_SORTED = 3;                     // the fourth class
constexpr int64_t LV_MAX_GRID = 2048;
constexpr uint32_t LV_NONE = 0xffffffffu;        // no entry here (past the row's end, or a self entry); sorts behind every community id
constexpr int64_t LV_M_LIMIT = (int64_t)1 << 31;
constexpr int64_t LV_NO_SCORE = INT64_MIN;       // below every score: |score| < 2^62

enum {
    LC_I = 0,           // sum over v of k(v, A) + the weight of v's self entries
    LC_S = 1,           // sum over c of tot[c]^2
    LC_W = 2,           // the vertices that want to move
    LC_APPLIED = 3,     // the moves the apply before this round's evaluation made
    LC_NEG = 4,         // entries of negative weight
    LC_M = 5,           // the sum of min(weight, 2^31) over the entries
    LC_COMMS = 6,       // communities of the level's result
    LC_ROWS = 7,        // + class: rows of length > 0 per class
    LC_SKEYS = 11,      // the entries of the sorted rows
    LC_TAIL = 12,       // + class: rows appended to the class list so far
    LC_NCNT = 15
};
static_assert(LC_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

bool lv_sharded(const vgl_hip_graph *g) { return g->row_begin != 0 || g->row_end != g->V; }
__host__ __device__ inline int lv_class_of(int64_t len, vgl_rc_bounds b, int32_t wg)
{
    if (len <= 0) return -1;
    const int k = vgl_rc_class_of(len, b);
    return k == VGL_RC_WG && len > wg ? LV_SORTED : k;
}
__host__ __device__ inline uint32_t lv_key(uint32_t i, uint32_t s) { return vgl_fmix32(i ^ vgl_fmix32(s + 0x9e3779b9u)); }

// what a round reads: the level's CSR with its weights (nullptr: 1 each), k, and the snapshot (comm, tot, size)
struct lv_view {
    int32_t V;
    int64_t m;
    const int64_t *rowptr;
    const int32_t *adj;
    const int64_t *w;
    const int64_t *k;
    const int32_t *comm;
    const int64_t *tot;
    const int32_t *size;
    __device__ __forceinline__ int64_t weight(int64_t p) const { return w ? w[p] : 1; }
};

// ---- level set-up ----
// k[v] += the weight of every entry of row v (k cleared before); the negative weights and the clamped total
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_degree(int32_t V, int64_t E, const int64_t *rowptr, const int64_t *w, int64_t *k, unsigned long long *cnt)
{
    int64_t neg = 0, m = 0;
    if (w) {
        for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < E; e += (int64_t)gridDim.x * VGL_BLOCK) {
            const int64_t x = w[e];
            neg += x < 0;
            m += x < 0 ? 0 : x < LV_M_LIMIT ? x : LV_M_LIMIT;
            if (x > 0) vgl_atomic_add64(k + vgl_row_of(rowptr, V, e), x);
        }
    } else {
        for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
            const int64_t d = rowptr[v + 1] - rowptr[v];
            k[v] = d;
            m += d;
        }
    }
    vgl_wave_flush_add(cnt + LC_NEG, neg);
    vgl_wave_flush_add(cnt + LC_M, m);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_init(int32_t V, const int64_t *k, int32_t *comm, int64_t *tot, int32_t *size, int32_t *best)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        comm[v] = (int32_t)v;
        tot[v] = k[v];
        size[v] = 1;
        best[v] = -1;
    }
}
struct lv_src {
    const int64_t *rowptr;
    vgl_rc_bounds b;
    int32_t wg;
    __device__ __forceinline__ int cls(int64_t i, int64_t &work) const
    {
        work = rowptr[i + 1] - rowptr[i];
        const int k = lv_class_of(work, b, wg);
        return k == LV_SORTED ? -1 : k;
    }
};
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_classify(lv_src s, int32_t V, unsigned long long *cnt)
{
    int64_t rows[4] = {0, 0, 0, 0}, skeys = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t len = s.rowptr[v + 1] - s.rowptr[v];
        const int k = lv_class_of(len, s.b, s.wg);
#pragma unroll
        for (int q = 0; q < 4; q++) rows[q] += k == q;
        skeys += k == LV_SORTED ? len : 0;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) vgl_wave_flush_add(cnt + LC_ROWS + q, rows[q]);
    vgl_wave_flush_add(cnt + LC_SKEYS, skeys);
}
// the sorted rows in ascending order: flags (V + 1, the last 0), their exclusive scan, the scatter
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_sorted_flag(lv_src s, int32_t V, int32_t *flag)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v <= V; v += (int64_t)gridDim.x * VGL_BLOCK)
        flag[v] = v < V && lv_class_of(s.rowptr[v + 1] - s.rowptr[v], s.b, s.wg) == LV_SORTED;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_sorted_list(lv_src s, int32_t V, const int32_t *flag, const int32_t *pos, int64_t nsorted, int32_t *srows, int64_t *slen)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK)
        if (flag[v] && pos[v] >= 0 && pos[v] < nsorted) {
            srows[pos[v]] = (int32_t)v;
            slen[pos[v]] = s.rowptr[v + 1] - s.rowptr[v];
        }
}

// ---- the pick, shared by the four classes ----
// Every lane of the team holds its best candidate other than A (score LV_NO_SCORE: none); kA and selfw are the team's sums.  The lead lane stores
// best[v] (the community v wants to move to, or -1) and adds to its partial sums of I and W.
template <class T>
__device__ __forceinline__ void lv_pick(const lv_view &a, int32_t v, bool has, int64_t bs, int32_t bc, int64_t kA, int64_t selfw, int32_t *best, int64_t &sumI, int64_t &sumW)
{
    const int64_t top = T::max_of(bs);
    const int32_t to = T::min_of(bs == top && top != LV_NO_SCORE ? bc : INT32_MAX);
    if (!T::lead() || !has) return;
    const int32_t A = a.comm[v];
    const int64_t kv = a.k[v];
    const int64_t scoreA = kA * a.m - kv * (a.tot[A] - kv);
    bool wants = top != LV_NO_SCORE && top > scoreA;
    if (wants && a.size[A] == 1 && a.size[to] == 1 && to > A) wants = false;      // the swap guard
    best[v] = wants ? to : -1;
    sumI += kA + selfw;
    sumW += wants;
}
template <int CLS>
__device__ __forceinline__ void lv_team_sync()
{
    if constexpr (CLS == VGL_RC_WG) __syncthreads();
    else {                                                            // one wavefront: its LDS operations complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}
__device__ __forceinline__ void lv_better(int64_t sc, int32_t c, int64_t &bs, int32_t &bc)
{
    if (sc > bs || (sc == bs && c < bc)) { bs = sc; bc = c; }
}

template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_eval(const int32_t *list, int32_t n, lv_view a, int32_t *best, unsigned long long *cnt)
{
    using T = vgl_rc_team<CLS>;
    int64_t sumI = 0, sumW = 0;
    if constexpr (CLS == VGL_RC_SHORT) {
        for (int64_t at0 = T::begin(); at0 < n; at0 += T::stride()) {
            const int64_t i = T::item(at0);
            const bool has = i < n;
            const int32_t v = has ? list[i] : 0;
            const int64_t s = has ? a.rowptr[v] : 0, len = has ? a.rowptr[v + 1] - s : 0;
            const int32_t A = has ? a.comm[v] : -1;
            const int64_t kv = has ? a.k[v] : 0;
            const int nch = (int)((len + T::LANES - 1) / T::LANES);
            int64_t bs = LV_NO_SCORE, kA = 0, selfw = 0;
            int32_t bc = INT32_MAX;
            for (int ca = 0; T::together(ca < nch); ca++) {
                const int64_t j = (int64_t)ca * T::LANES + T::lane();
                uint32_t mine = LV_NONE;
                if (j < len) {
                    const int32_t far = a.adj[s + j];
                    const int64_t wj = a.weight(s + j);
                    if (far == v) selfw += wj;
                    else {
                        mine = (uint32_t)a.comm[far];
                        if ((int32_t)mine == A) kA += wj;
                    }
                }
                bool head = mine != LV_NONE && (int32_t)mine != A;
                int64_t sum = 0;
                for (int cb = 0; T::together(cb < nch); cb++) {
                    const int64_t jb = (int64_t)cb * T::LANES + T::lane();
                    uint32_t kb = LV_NONE;
                    int64_t wb = 0;
                    if (jb < len) {
                        const int32_t far = a.adj[s + jb];
                        if (far != v) { kb = (uint32_t)a.comm[far]; wb = a.weight(s + jb); }
                    }
#pragma unroll
                    for (int l = 0; l < T::LANES; l++) {
                        const uint32_t other = __shfl(kb, l, T::LANES);
                        const long long ow = __shfl((long long)wb, l, T::LANES);
                        if (other == mine) {
                            sum += ow;
                            if ((int64_t)cb * T::LANES + l < j) head = false;
                        }
                    }
                }
                if (head) lv_better(sum * a.m - kv * a.tot[mine], (int32_t)mine, bs, bc);
            }
            kA = T::sum_of(kA);
            selfw = T::sum_of(selfw);
            lv_pick<T>(a, v, has, bs, bc, kA, selfw, best, sumI, sumW);
        }
    } else {
        constexpr int CAP = CLS == VGL_RC_WAVE ? LV_WAVE_CAP : LV_WG_CAP;
        __shared__ uint32_t s_keys[T::ITEMS_PER_WG][CAP];
        __shared__ int64_t s_sum[T::ITEMS_PER_WG][CAP];
        uint32_t *K = s_keys[T::team()];
        int64_t *S = s_sum[T::team()];
        for (int64_t i = T::begin(); i < n; i += T::stride()) {       // (uniform over the team)
            const int32_t v = list[i];
            const int64_t s = a.rowptr[v];
            int64_t len = a.rowptr[v + 1] - s;
            if (len > CAP) len = 0;                                   // (never: the bounds are clamped on the host)
            const int32_t A = a.comm[v];
            const int64_t kv = a.k[v];
            int P = 1;
            while (P < len) P <<= 1;
            lv_team_sync<CLS>();                                      // the item before has been read
            for (int x = T::lane(); x < P; x += T::LANES) {
                uint32_t key = LV_NONE;
                if (x < len) {
                    const int32_t far = a.adj[s + x];
                    if (far != v) key = (uint32_t)a.comm[far];
                }
                K[x] = key;
            }
            lv_team_sync<CLS>();
            for (int k = 2; k <= P; k <<= 1)                          // bitonic sort, ascending: LV_NONE ends up behind the community ids
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int x = T::lane(); x < P; x += T::LANES) {
                        const int y = x ^ j;
                        if (y > x) {
                            const uint32_t kx = K[x], ky = K[y];
                            if ((kx > ky) == ((x & k) == 0)) { K[x] = ky; K[y] = kx; }
                        }
                    }
                    lv_team_sync<CLS>();
                }
            // the distinct keys move to K[0, d) in order: a head at x goes to a slot <= x, and only to x itself when nothing before it was dropped
            int d = 0;
            for (int x0 = 0; x0 < P; x0 += T::LANES) {                // (uniform over the team)
                const int x = x0 + T::lane();
                const uint32_t kx = x < P ? K[x] : LV_NONE;
                const bool head = kx != LV_NONE && (x == 0 || K[x - 1] != kx);
                lv_team_sync<CLS>();
                int tot = 0;
                const int rank = T::rank(head, &tot);
                if (head) K[d + rank] = kx;
                d += tot;
                lv_team_sync<CLS>();
            }
            for (int x = T::lane(); x < d; x += T::LANES) S[x] = 0;
            lv_team_sync<CLS>();
            int64_t selfw = 0;
            for (int64_t j = T::lane(); j < len; j += T::LANES) {
                const int32_t far = a.adj[s + j];
                const int64_t wj = a.weight(s + j);
                if (far == v) { selfw += wj; continue; }
                const uint32_t kj = (uint32_t)a.comm[far];
                int lo = 0, hi = d;                                   // the first slot whose key is not below kj
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (K[mid] < kj) lo = mid + 1; else hi = mid;
                }
                if (lo < d) atomicAdd(reinterpret_cast<unsigned long long *>(S + lo), (unsigned long long)wj);
            }
            lv_team_sync<CLS>();
            int64_t bs = LV_NO_SCORE, kA = 0;
            int32_t bc = INT32_MAX;
            for (int x = T::lane(); x < d; x += T::LANES) {
                const uint32_t c = K[x];
                if ((int32_t)c == A) kA = S[x];
                else lv_better(S[x] * a.m - kv * a.tot[c], (int32_t)c, bs, bc);
            }
            kA = T::sum_of(kA);                                       // (one lane holds it)
            selfw = T::sum_of(selfw);
            lv_pick<T>(a, v, true, bs, bc, kA, selfw, best, sumI, sumW);
        }
    }
    vgl_wave_flush_add(cnt + LC_I, sumI);
    vgl_wave_flush_add(cnt + LC_W, sumW);
}

// ---- the sorted class ----
// key t of the piece: flat entry f0 + t of the sorted rows [i0, i1)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_emit(lv_view a, const int32_t *srows, const int64_t *soff, int64_t i0, int64_t i1, int64_t nk, uint64_t *keys, int64_t *vals)
{
    const int64_t f0 = soff[i0];
    for (int64_t t = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; t < nk; t += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t f = f0 + t;
        int64_t lo = i0, hi = i1;                                     // invariant: soff[lo] <= f < soff[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (soff[mid] <= f) lo = mid; else hi = mid;
        }
        const int32_t v = srows[lo];
        const int64_t p = a.rowptr[v] + (f - soff[lo]);
        const int32_t far = a.adj[p];
        keys[t] = (uint64_t)(uint32_t)v << 32 | (far == v ? LV_NONE : (uint32_t)a.comm[far]);
        vals[t] = a.weight(p);
    }
}
// a wavefront per sorted row of the piece: the runs of row v start at the first key not below v << 32
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_score(lv_view a, const int32_t *srows, int64_t i0, int64_t i1, const uint64_t *ukeys, const int64_t *usums,
                                                                 const int64_t *n_unique, int64_t nk, int32_t *best, unsigned long long *cnt)
{
    using T = vgl_rc_team<VGL_RC_WAVE>;
    const int64_t n = *n_unique < nk ? *n_unique : nk;
    int64_t sumI = 0, sumW = 0;
    for (int64_t i = i0 + T::begin(); i < i1; i += T::stride()) {     // (uniform over the wave)
        const int32_t v = srows[i];
        const int32_t A = a.comm[v];
        const int64_t kv = a.k[v];
        const uint64_t first = (uint64_t)(uint32_t)v << 32;
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (ukeys[mid] < first) lo = mid + 1; else hi = mid;
        }
        int64_t bs = LV_NO_SCORE, kA = 0, selfw = 0;
        int32_t bc = INT32_MAX;
        for (int64_t x0 = lo; x0 < n; x0 += 64) {                     // (uniform over the wave)
            const int64_t x = x0 + T::lane();
            const uint64_t key = x < n ? ukeys[x] : ~0ull;
            const bool in = x < n && (key >> 32) == (uint64_t)(uint32_t)v;
            if (in) {
                const uint32_t c = (uint32_t)key;
                if (c == LV_NONE) selfw = usums[x];
                else if ((int32_t)c == A) kA = usums[x];
                else lv_better(usums[x] * a.m - kv * a.tot[c], (int32_t)c, bs, bc);
            }
            if (!__all(in)) break;
        }
        kA = T::sum_of(kA);
        selfw = T::sum_of(selfw);
        lv_pick<T>(a, v, true, bs, bc, kA, selfw, best, sumI, sumW);
    }
    vgl_wave_flush_add(cnt + LC_I, sumI);
    vgl_wave_flush_add(cnt + LC_W, sumW);
}

// ---- reduce, apply, count ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_sumsq(int32_t V, const int64_t *tot, unsigned long long *cnt)
{
    int64_t s = 0;
    for (int64_t c = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; c < V; c += (int64_t)gridDim.x * VGL_BLOCK) s += tot[c] * tot[c];
    vgl_wave_flush_add(cnt + LC_S, s);
}
// next = the snapshot with the moves of the active half applied; tot and size of next (cleared before) are recounted
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_apply(int32_t V, uint32_t round_seed, const int64_t *k, const int32_t *comm, const int32_t *best, int32_t *next,
                                                                 int64_t *tot, int32_t *size, unsigned long long *cnt)
{
    int64_t moved = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t to = best[v];
        const bool go = to >= 0 && to < V && (lv_key((uint32_t)v, round_seed) & 1u);
        const int32_t c = go ? to : comm[v];
        next[v] = c;
        moved += go;
        const int64_t kv = k[v];
        if (kv) vgl_atomic_add64(tot + c, kv);
        atomicAdd(size + c, 1);
    }
    vgl_wave_flush_add(cnt + LC_APPLIED, moved);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_louvain_count(int32_t V, const int32_t *size, unsigned long long *cnt)
{
    int64_t s = 0;
    for (int64_t c = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; c < V; c += (int64_t)gridDim.x * VGL_BLOCK) s += size[c] > 0;
    vgl_wave_flush_add(cnt + LC_COMMS, s);
}
struct lv_params {
    int32_t max_rounds;
    int64_t D;
    vgl_rc_bounds b;
    int32_t wg;
    int64_t cap_keys;
};
struct lv_level {
    int64_t m = 0, N = 0, communities = 0, rows[4] = {0, 0, 0, 0}, skeys = 0, pieces = 0;
    int32_t rounds = 0, outcome = 0;
};

int lv_params_of(vgl_hip_ctx *c, int32_t max_rounds, int64_t D, lv_params *p)
{
    p->max_rounds = max_rounds;
    p->D = D;
    p->b = vgl_rc_env_bounds(c, "VGL_LOUVAIN_SHORT", "VGL_LOUVAIN_WAVE");
    p->b.wave = std::min<int32_t>(p->b.wave, LV_WAVE_CAP);
    p->b.shrt = std::min(p->b.shrt, p->b.wave);
    p->wg = (int32_t)vgl_env_int(c, "VGL_LOUVAIN_WG", LV_WG_CAP, p->b.wave, LV_WG_CAP);
    const int64_t cap_mb = vgl_env_int(c, "VGL_LOUVAIN_SORT_CAP_MB", 4096, 0, (int64_t)1 << 24);
    p->cap_keys = cap_mb == 0 ? INT64_MAX : (cap_mb << 20) / 32;      // keys in and out, sums in and out: 32 bytes per key
    return 0;
}

const int64_t lv_grid_cap[VGL_RC_N] = {4 * LV_MAX_GRID, 4 * LV_MAX_GRID, 4 * LV_MAX_GRID};

// One level over a borrowed CSR (V >= 1; w: nullptr = 1 each): the result goes to d_result (int32, V, device), what the host knows of it to *out.
// Fails on a negative weight and on m >= 2^31 before d_result is written.
int lv_move(vgl_hip_ctx *c, int32_t V, int64_t E, const int64_t *rowptr, const int32_t *adj, const int64_t *w, const lv_params &P, uint32_t seed, int32_t *d_result, lv_level *out)
{
    hipStream_t st = c->stream;
    const unsigned grid_v = vgl_grid(V, VGL_BLOCK, LV_MAX_GRID), grid_e = vgl_grid(E, VGL_BLOCK, 4 * LV_MAX_GRID);
    vgl_dev<unsigned long long> cnt;
    vgl_dev<int64_t> k, tot[2];
    vgl_dev<int32_t> comm[2], size[2], best;
    VGL_TRY(vgl_open_counters(c, &cnt, LC_NCNT));
    VGL_TRY(k.alloc(st, (size_t)V));
    VGL_TRY(best.alloc(st, (size_t)V));
    for (int x = 0; x < 2; x++) {
        VGL_TRY(tot[x].alloc(st, (size_t)V));
        VGL_TRY(comm[x].alloc(st, (size_t)V));
        VGL_TRY(size[x].alloc(st, (size_t)V));
    }
    VGL_HIP_TRY(hipMemsetAsync(k.p, 0, sizeof(int64_t) * (size_t)V, st));
    const lv_src src{rowptr, P.b, P.wg};
    {
        vgl_timed_launch tl(c, "louvain_prepare");
        hipLaunchKernelGGL(vgl_k_louvain_degree, dim3(w ? grid_e : grid_v), dim3(VGL_BLOCK), 0, st, V, E, rowptr, w, k.p, cnt.p);
        hipLaunchKernelGGL(vgl_k_louvain_classify, dim3(grid_v), dim3(VGL_BLOCK), 0, st, src, V, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_publish_counters(c, "louvain_publish", cnt, LC_NCNT));
    if (c->h_counters[LC_NEG] != 0) VGL_FAIL("louvain: a weight is negative");
    const int64_t m = c->h_counters[LC_M];
    if (m < 0 || m >= LV_M_LIMIT) VGL_FAIL("louvain: the total weight m (the sum over all slots) is 2^31 or more");
    lv_level L;
    L.m = m;
    int64_t total = 0;
    for (int q = 0; q < 4; q++) {
        L.rows[q] = c->h_counters[LC_ROWS + q];
        if (L.rows[q] < 0) VGL_FAIL("louvain: internal error (a class count is negative)");
        total += L.rows[q];
    }
    L.skeys = c->h_counters[LC_SKEYS];
    if (total > V || L.skeys < 0 || L.skeys > E) VGL_FAIL("louvain: internal error (the classes exceed the rows)");
    {
        vgl_timed_launch tl(c, "louvain_prepare");
        hipLaunchKernelGGL(vgl_k_louvain_init, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const int64_t *)k.p, comm[0].p, tot[0].p, size[0].p, best.p);
    }
    VGL_HIP_TRY(hipGetLastError());

    // the class lists, the sorted rows and their pieces
    vgl_rc_lists<vgl_rc_bounded> lists;
    for (int q = 0; q < VGL_RC_N; q++) lists.rows[q] = L.rows[q];
    VGL_TRY(lists.fill(c, "louvain_prepare", src, V, LV_MAX_GRID, 1, nullptr, cnt + LC_TAIL));
    const int64_t nsorted = L.rows[LV_SORTED];
    vgl_dev<int32_t> srows;
    vgl_dev<int64_t> soff;
    std::vector<int64_t> soff_h, piece;
    int64_t piece_keys = 0;
    vgl_dev<uint64_t> keys_a, keys_b;
    vgl_dev<int64_t> vals_a, vals_b, n_unique;
    vgl_scratch temp;
    const int end_bit = 32 + vgl_index_bits(V);
    if (nsorted > 0) {
        vgl_dev<int32_t> flag, pos;
        vgl_dev<int64_t> slen;
        VGL_TRY(flag.alloc(st, (size_t)V + 1));
        VGL_TRY(pos.alloc(st, (size_t)V + 1));
        VGL_TRY(slen.alloc(st, (size_t)nsorted + 1));
        VGL_TRY(srows.alloc(st, (size_t)nsorted));
        VGL_TRY(soff.alloc(st, (size_t)nsorted + 1));
        vgl_scratch tmp;
        VGL_TRY(vgl_exclusive_scan(c, tmp, flag.p, pos.p, (size_t)V + 1, VGL_SIZE_ONLY));
        VGL_TRY(vgl_exclusive_scan(c, tmp, slen.p, soff.p, (size_t)nsorted + 1, VGL_SIZE_ONLY));
        VGL_HIP_TRY(hipMemsetAsync(slen.p + nsorted, 0, sizeof(int64_t), st));
        {
            vgl_timed_launch tl(c, "louvain_prepare");
            hipLaunchKernelGGL(vgl_k_louvain_sorted_flag, dim3(grid_v), dim3(VGL_BLOCK), 0, st, src, V, flag.p);
            VGL_TRY(vgl_exclusive_scan(c, tmp, flag.p, pos.p, (size_t)V + 1));
            hipLaunchKernelGGL(vgl_k_louvain_sorted_list, dim3(grid_v), dim3(VGL_BLOCK), 0, st, src, V, (const int32_t *)flag.p, (const int32_t *)pos.p, nsorted, srows.p, slen.p);
            VGL_TRY(vgl_exclusive_scan(c, tmp, slen.p, soff.p, (size_t)nsorted + 1));
        }
        VGL_HIP_TRY(hipGetLastError());
        soff_h.assign((size_t)nsorted + 1, 0);
        VGL_HIP_TRY(hipMemcpyAsync(soff_h.data(), soff.p, sizeof(int64_t) * ((size_t)nsorted + 1), hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (soff_h[(size_t)nsorted] != L.skeys) VGL_FAIL("louvain: internal error (the sorted rows do not add up)");
        for (int64_t i = 0; i < nsorted; i++)
            if (soff_h[(size_t)i + 1] <= soff_h[(size_t)i]) VGL_FAIL("louvain: internal error (a sorted row is empty)");
        piece_keys = vgl_plan_pieces(nsorted, [&](int64_t i) { return soff_h[(size_t)i + 1] - soff_h[(size_t)i]; }, P.cap_keys, &piece);
        L.pieces = (int64_t)piece.size() - 1;
        const size_t cap = (size_t)std::max<int64_t>(piece_keys, 1);
        VGL_TRY(keys_a.alloc(st, cap));
        VGL_TRY(keys_b.alloc(st, cap));
        VGL_TRY(vals_a.alloc(st, cap));
        VGL_TRY(vals_b.alloc(st, cap));
        VGL_TRY(n_unique.alloc(st, 1));
        VGL_TRY(vgl_sort_pairs(c, temp, keys_a.p, keys_b.p, vals_a.p, vals_b.p, cap, 0, end_bit, VGL_SIZE_ONLY));      // sized here for the largest piece
        VGL_TRY(vgl_reduce_by_key(c, temp, keys_b.p, vals_b.p, cap, keys_a.p, vals_a.p, n_unique.p, VGL_SIZE_ONLY));
    }

    const char *const eval_slot[VGL_RC_N] = {"louvain_eval_short", "louvain_eval_wave", "louvain_eval_wg"};
    const int32_t *const list[VGL_RC_N] = {lists.l[0].rows, lists.l[1].rows, lists.l[2].rows};
    const int64_t m2_over_D = P.D > 0 ? (m * m) / P.D : 0;
    int cur = 0;                                                      // the snapshot; after an apply, 1 - cur holds the assignment before it
    int64_t N_kept = 0;
    int result = 0;
    for (int32_t r = 1;; r++) {
        VGL_HIP_TRY(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * 4, st));
        if (r > 1) {                                                  // the moves of round r - 1
            const int nx = 1 - cur;
            VGL_HIP_TRY(hipMemsetAsync(tot[nx].p, 0, sizeof(int64_t) * (size_t)V, st));
            VGL_HIP_TRY(hipMemsetAsync(size[nx].p, 0, sizeof(int32_t) * (size_t)V, st));
            {
                vgl_timed_launch tl(c, "louvain_apply");
                hipLaunchKernelGGL(vgl_k_louvain_apply, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, seed + (uint32_t)(r - 1), (const int64_t *)k.p, (const int32_t *)comm[cur].p,
                                   (const int32_t *)best.p, comm[nx].p, tot[nx].p, size[nx].p, cnt.p);
            }
            cur = nx;
        }
        const lv_view a{V, m, rowptr, adj, w, k.p, comm[cur].p, tot[cur].p, size[cur].p};
        VGL_TRY(vgl_rc_launch_trio(c, eval_slot, lists.rows, lv_grid_cap, vgl_k_louvain_eval<VGL_RC_SHORT>, vgl_k_louvain_eval<VGL_RC_WAVE>, vgl_k_louvain_eval<VGL_RC_WG>, list, a, best.p,
                                   cnt.p));
        for (size_t pc = 0; pc + 1 < piece.size() && nsorted > 0; pc++) {
            const int64_t i0 = piece[pc], i1 = piece[pc + 1], nk = soff_h[(size_t)i1] - soff_h[(size_t)i0];
            if (nk <= 0 || nk > std::max<int64_t>(piece_keys, 1)) VGL_FAIL("louvain: internal error (a sort piece does not fit its buffers)");
            vgl_timed_launch tl(c, "louvain_eval_sorted");
            hipLaunchKernelGGL(vgl_k_louvain_emit, dim3(vgl_grid(nk, VGL_BLOCK, 4 * LV_MAX_GRID)), dim3(VGL_BLOCK), 0, st, a, (const int32_t *)srows.p, (const int64_t *)soff.p, i0, i1, nk,
                               keys_a.p, vals_a.p);
            VGL_TRY(vgl_sort_pairs(c, temp, keys_a.p, keys_b.p, vals_a.p, vals_b.p, (size_t)nk, 0, end_bit));
            VGL_TRY(vgl_reduce_by_key(c, temp, keys_b.p, vals_b.p, (size_t)nk, keys_a.p, vals_a.p, n_unique.p));
            hipLaunchKernelGGL(vgl_k_louvain_score, dim3(vgl_grid(i1 - i0, VGL_WAVES, 4 * LV_MAX_GRID)), dim3(VGL_BLOCK), 0, st, a, (const int32_t *)srows.p, i0, i1,
                               (const uint64_t *)keys_a.p, (const int64_t *)vals_a.p, (const int64_t *)n_unique.p, nk, best.p, cnt.p);
        }
        {
            vgl_timed_launch tl(c, "louvain_reduce");
            hipLaunchKernelGGL(vgl_k_louvain_sumsq, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const int64_t *)tot[cur].p, cnt.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(vgl_publish_counters(c, "louvain_publish", cnt, 4));
        const int64_t I = c->h_counters[LC_I], S = c->h_counters[LC_S], W = c->h_counters[LC_W], applied = c->h_counters[LC_APPLIED];
        const int64_t N = m * I - S;
        L.rounds = r;
        result = cur;
        if (r > 1 && applied > 0 && N <= N_kept) {                    // the round before made it no better: its moves are dropped
            L.outcome = VGL_HIP_LOUVAIN_REVERTED;
            result = 1 - cur;
            break;
        }
        const int64_t before = N_kept;
        N_kept = N;
        if (P.D > 0 && r > 1 && applied > 0 && N - before < m2_over_D) { L.outcome = VGL_HIP_LOUVAIN_SMALL_GAIN; break; }
        if (W == 0) { L.outcome = VGL_HIP_LOUVAIN_CONVERGED; break; }
        if (r == P.max_rounds) { L.outcome = VGL_HIP_LOUVAIN_CAPPED; break; }
    }
    L.N = N_kept;
    {
        vgl_timed_launch tl(c, "louvain_reduce");
        hipLaunchKernelGGL(vgl_k_louvain_count, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)size[result].p, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_publish_counters(c, "louvain_publish", cnt, LC_NCNT));
    L.communities = c->h_counters[LC_COMMS];
    if (L.communities < 1 || L.communities > V) VGL_FAIL("louvain: internal error (the communities exceed the vertices)");
    VGL_HIP_TRY(hipMemcpyAsync(d_result, comm[result].p, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToDevice, st));
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // the level's buffers are freed on return
    *out = L;
    return 0;
}

// the bytes of one level (include/vgl_hip.h has the terms); wb = 8 when the level reads weights
int64_t lv_level_bytes(int64_t V, int64_t E, int64_t rounds, int64_t wb)
{
    return 8 * (V + 1) + (4 + wb) * E + 24 * V + rounds * ((8 + wb) * E + 44 * V) + (rounds - 1) * 32 * V;
}
void lv_note_level(vgl_hip_louvain_stats *s, int l, int64_t V, int64_t E, const lv_level &L, int64_t wb)
{
    s->vertices[l] = V;
    s->entries[l] = E;
    s->communities[l] = L.communities;
    s->rounds[l] = L.rounds;
    s->outcome[l] = L.outcome;
    s->level_modularity_num[l] = L.N;
    s->entries_walked += (int64_t)L.rounds * E;
    s->algorithmic_bytes += lv_level_bytes(V, E, L.rounds, wb);
    if (l == 0) {
        s->total_weight = L.m;
        s->rows_short = L.rows[0]; s->rows_wave = L.rows[1]; s->rows_wg = L.rows[2]; s->rows_sorted = L.rows[3];
        s->sorted_keys = L.skeys;
        s->sort_pieces = L.pieces;
    }
    s->modularity_num = L.N;
    s->levels = l + 1;
}
int lv_check_rounds(int32_t max_rounds, int64_t D)
{
    if (max_rounds < 1 || max_rounds > 65535) VGL_FAIL("louvain: max_rounds must be in [1, 65535]");
    if (D < 0) VGL_FAIL("louvain: min_gain_den must not be negative");
    return 0;
}

}  // namespace

extern "C" {

int vgl_hip_louvain_move(vgl_hip_ctx *c, vgl_hip_graph *g, const int64_t *d_weight, int32_t max_rounds, int64_t min_gain_den, uint32_t seed, int32_t *d_label,
                         vgl_hip_louvain_stats *stats)
{
    if (!c || !g || !d_label) VGL_FAIL("louvain_move: null argument");
    if (lv_sharded(g)) VGL_FAIL("louvain_move: graph handle must own all rows (louvain has no sharded form)");
    VGL_TRY(lv_check_rounds(max_rounds, min_gain_den));
    vgl_hip_louvain_stats s;
    memset(&s, 0, sizeof(s));
    if (g->V < 1) {
        if (stats) *stats = s;
        return 0;
    }
    lv_params P;
    VGL_TRY(lv_params_of(c, max_rounds, min_gain_den, &P));
    vgl_dev<int32_t> result;
    VGL_TRY(result.alloc(c->stream, (size_t)g->V));
    lv_level L;
    VGL_TRY(lv_move(c, g->V, g->out.edges, g->out.rowptr, g->out.adj, d_weight, P, seed, result.p, &L));
    lv_note_level(&s, 0, g->V, g->out.edges, L, d_weight ? 8 : 0);
    VGL_HIP_TRY(hipMemcpyAsync(d_label, result.p, sizeof(int32_t) * (size_t)g->V, hipMemcpyDeviceToDevice, c->stream));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) *stats = s;
    return 0;
}

}  // extern "C"
