// msbfs.hip -- bit-parallel multi-source BFS (MS-BFS; Then et al., VLDB 2014) of the stored directed, unweighted graph, 64 sources per batch, and the
// per-source sums closeness, harmonic centrality and eccentricity are made of.  The contract is written out in include/vgl_hip.h; DESIGN section 19
// has the schedule, the kernel resources and the bytes model.
//
// Per batch every vertex carries three 64-bit words, bit b = source b of the batch: seen (bits that have reached the vertex), cur (bits that arrived
// with the frontier about to be expanded) and nxt (bits arriving now).  The frontier is also a list of the vertices with a non-zero cur word, one
// list per row class of the traversal direction, so that a level costs its entries and not V.
//   seed     one workgroup: cur[s] |= 1ull << b and seen[s] |= 1ull << b by 64-bit atomic ORs (two sources may share a vertex); the thread that
//            found the word empty lists the vertex.
//   push     over the current lists, one kernel per row class (short: 8 lanes per row, wave: a wavefront, wg: a workgroup per chunk).  For an
//            entry (v -> w): add = cur[v] & ~seen[w]; a non-zero add goes to nxt[w] by atomicOr, and the lane that saw the word empty appends w.
//   pull     over ALL rows of the reverse CSR, by its row classes: want = active & ~seen[v] (active = the batch's live bits); a row with want == 0
//            is not read; otherwise acc |= cur[u] over the entries until acc covers want; nxt[v] = acc & want, one writer (a row longer than a
//            wave's class is cut into chunks, whose workgroups combine by atomicOr on that row's word), a non-zero result appends v.
//   settle   over the next lists only: seen[v] |= nxt[v], the degree of v into the frontier-entries counter, the level into d_levels for every set
//            bit, and the per-source counts by the wave-64 transpose (lane b adds popcount(ballot(bit b)): 64 ballots per 64 vertices, no LDS
//            atomics, then one integer atomic per lane and wave).  The old frontier's cur words are cleared through the old lists, and the two
//            word arrays change roles on the host: what was nxt is cur, what was cur is all zero and is nxt.
//   publish  64 threads: the per-source count c of distance d goes into reached, dist_sum, ecc and harmonic (h = h + (double)c / (double)d: one writer,
//            one division and one addition per level in ascending d, no floating-point atomics), the counters go to the pinned mirror and are zeroed:
//            one host read per level.
// Appends are staged per wave in LDS and cost one returning atomic per 64 or more vertices.
// INVARIANT: inside one launch no word that another workgroup of that launch writes is read with a plain load.  seen and cur are constant within push
// and pull; nxt is touched only by atomics in push, and in pull only by its single writer (short and wave rows) or only by atomics (chunked rows);
// settle reads nxt and the list tails, which the launch before it wrote, writes seen[v] for the listed v alone, and clears the OTHER word array.
// Everything else crosses a kernel boundary.  No cooperative launch, no grid barrier, no spin on a flag.
#include "vgl_rowclass.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

typedef unsigned long long ms_word;
constexpr int MS_BATCH = 64;                     // sources per batch: one bit each
constexpr int64_t MS_MAX_GRID = 2048;            // workgroups of a grid-stride kernel
enum {
    MS_TAIL = 0,        // + class: vertices appended to the next list of the class by this level
    MS_ENTRIES = 3,     // traversal-direction degrees of the next frontier's vertices
    MS_BITS = 4,        // (vertex, source) pairs the level reached
    MS_PULLED = 5,      // entries a pull level examined
    MS_NPUB = 6,        // what the host reads per level
    MS_SRC = 8,         // + bit: vertices the level reached for that source
    MS_NCNT = MS_SRC + MS_BATCH
};
static_assert(MS_NPUB <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

// the lists of one frontier: one per row class of the traversal direction, cap[c] = rows of the class
struct ms_lists { int32_t *rows[VGL_RC_N]; int32_t cap[VGL_RC_N]; };
// where a level appends: the next lists, the class of every vertex in the traversal direction, the counters
struct ms_out { ms_lists next; const uint8_t *cls; ms_word *cnt; };
// one level: the CSR it walks (push: the traversal direction; pull: its reverse) and the words
struct ms_level {
    const int64_t *rowptr;
    const int32_t *adj;
    vgl_rc_chunks ch;            // of that CSR's workgroup rows
    const ms_word *cur, *seen;
    ms_word *nxt;
    ms_word active;              // pull: the batch's live bits
    ms_out out;
};

// ---- prepare: the class of every row of one direction, the class sizes, the longest row; then the rows by class ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msbfs_classify(int32_t V, const int64_t *rowptr, vgl_rc_bounds b, uint8_t *cls, ms_word *sizes, ms_word *max_row)
{
    int64_t n[VGL_RC_N] = {0, 0, 0};
    ms_word m = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t d = rowptr[v + 1] - rowptr[v];
        const int k = vgl_rc_class_of(d, b);
        cls[v] = (uint8_t)k;
        n[k]++;
        m = max(m, (ms_word)max(d, (int64_t)0));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if (vgl_lane() == 0 && m) atomicMax(max_row, m);
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) vgl_wave_flush_add(sizes + c, n[c]);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msbfs_rows(int32_t V, const uint8_t *cls, int32_t *r0, int32_t *r1, int32_t *r2, ms_word *tail)
{
    int32_t *const lists[VGL_RC_N] = {r0, r1, r2};
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < V; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t v = base + threadIdx.x;
        const bool want = v < V;
        vgl_wave_append<VGL_RC_N>(want, (int32_t)v, want ? (int)cls[v] : 0, lists, V, tail);
    }
}

// ---- the append staging: one vgl_rc_stage per class, onto the next lists (a list drops what runs past its end) ----
__device__ __forceinline__ vgl_rc_bounded ms_next(const ms_out &o, int c) { return vgl_rc_bounded{o.next.rows[c], o.next.cap[c]}; }
// every lane of the wave: the lanes with `app` append v to the next list of v's class
__device__ __forceinline__ void ms_append(vgl_rc_stage *st, bool app, int32_t v, const ms_out &o)
{
    if (!__any(app)) return;                                          // (uniform)
    const int k = app ? (int)o.cls[v] : -1;
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) st[c].keep(k == c, v, ms_next(o, c), o.cnt + MS_TAIL + c);
}
__device__ __forceinline__ void ms_flush_all(vgl_rc_stage *st, const ms_out &o)
{
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) st[c].flush(ms_next(o, c), o.cnt + MS_TAIL + c);
}

// ---- seed ----
__global__ __launch_bounds__(MS_BATCH) void vgl_k_msbfs_seed(const int32_t *src, int32_t nb, int32_t base, int32_t V, const int64_t *rowptr, ms_word *cur, ms_word *seen, ms_lists first,
                                                              const uint8_t *cls, ms_word *cnt, int64_t *reached, int64_t *dist_sum, int32_t *ecc, double *harmonic, int32_t *levels)
{
    __shared__ int s_tail[VGL_RC_N];
    __shared__ ms_word s_entries;
    const int b = threadIdx.x;
    if (b < VGL_RC_N) s_tail[b] = 0;
    if (b == 0) s_entries = 0;
    __syncthreads();
    if (b < nb) {
        const int32_t v = src[base + b];
        const ms_word bit = 1ull << b;
        const ms_word old = atomicOr(cur + v, bit);
        atomicOr(seen + v, bit);
        if (old == 0) {                                               // the first bit on this vertex lists it
            const int k = cls[v];
#pragma unroll
            for (int c = 0; c < VGL_RC_N; c++)
                if (k == c) {
                    const int pos = atomicAdd(&s_tail[c], 1);
                    if (pos < first.cap[c]) first.rows[c][pos] = v;
                }
            atomicAdd(&s_entries, (ms_word)(rowptr[v + 1] - rowptr[v]));
        }
        if (reached) reached[base + b] = 1;
        if (dist_sum) dist_sum[base + b] = 0;
        if (ecc) ecc[base + b] = 0;
        if (harmonic) harmonic[base + b] = 0.0;
        if (levels) levels[(int64_t)(base + b) * V + v] = 1;
    }
    __syncthreads();
    if (b < VGL_RC_N) cnt[MS_TAIL + b] = (ms_word)s_tail[b];
    if (b == 0) cnt[MS_ENTRIES] = s_entries;
}

// ---- push and pull: one team kernel each (short: 8 lanes per row, wave: a wavefront, workgroup: a workgroup per chunk of the row) ----
// one entry of row v (its frontier word cv): the bits the far end has not seen go to its nxt word; true for the lane that found the word empty
__device__ __forceinline__ bool ms_push_entry(const ms_level &t, ms_word cv, int32_t w)
{
    const ms_word add = cv & ~t.seen[w];
    return add != 0 && atomicOr(t.nxt + w, add) == 0;
}
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msbfs_push(const int32_t *rows, int32_t n, ms_level t)
{
    using T = vgl_rc_team<CLS>;
    vgl_rc_stage st[VGL_RC_N];
    vgl_rc_stage_open(st);
    const int64_t items = T::items(n, t.ch);
    for (int64_t at = T::begin(); at < items; at += T::stride()) {
        const int64_t i = T::item(at);
        ms_word cv = 0;
        int64_t lo = 0, hi = 0;
        if (i < items) {
            int64_t row;
            const int64_t k = T::piece(i, t.ch, &row);
            const int32_t v = rows[row];
            if (T::range(t.ch, t.rowptr[v], t.rowptr[v + 1], k, &lo, &hi)) cv = t.cur[v];
        }
        for (int64_t e0 = lo; T::together(e0 < hi); e0 += T::LANES) {  // (uniform over the wave)
            const int64_t e = e0 + T::lane();
            int32_t w = 0;
            bool app = false;
            if (e < hi) { w = t.adj[e]; app = ms_push_entry(t, cv, w); }
            ms_append(st, app, w, t.out);
        }
    }
    ms_flush_all(st, t.out);
}
// Short and wave rows have one writer and a staged append.  The pieces of a chunked row combine on its nxt word by atomicOr, and the one that found the
// word empty appends the row.  A wave leaves its row as soon as it covers `want`: the short form lane by lane, the others after the wave's or.
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msbfs_pull(const int32_t *rows, int32_t n, ms_level t)
{
    using T = vgl_rc_team<CLS>;
    const auto word_or = [](ms_word a, ms_word b) { return a | b; };
    vgl_rc_stage st[VGL_RC_N];
    if constexpr (CLS != VGL_RC_WG) vgl_rc_stage_open(st);
    const int64_t items = T::items(n, t.ch);
    int64_t examined = 0;
    for (int64_t at = T::begin(); at < items; at += T::stride()) {
        const int64_t i = T::item(at);
        int32_t v = 0;
        ms_word want = 0, acc = 0;
        int64_t k = 0, lo, hi;
        if (i < items) {
            int64_t row;
            k = T::piece(i, t.ch, &row);
            v = rows[row];
            want = t.active & ~t.seen[v];
        }
        const bool walk = want != 0 && T::range(t.ch, t.rowptr[v], t.rowptr[v + 1], k, &lo, &hi);
        if constexpr (CLS == VGL_RC_WG)
            if (!walk) continue;                                      // (uniform over the workgroup)
        if (walk) {
            if constexpr (CLS == VGL_RC_SHORT) {
                for (int64_t e = lo + T::lane(); e < hi; e += T::LANES) {      // (lane by lane)
                    acc |= t.cur[t.adj[e]];
                    examined++;
                    if ((acc & want) == want) break;
                }
            } else {
                for (int64_t e0 = lo; e0 < hi; e0 += T::LANES) {       // (uniform over the wave)
                    const int64_t e = e0 + T::lane();
                    if (e < hi) { acc |= t.cur[t.adj[e]]; examined++; }
                    acc = vgl_rc_team<VGL_RC_WAVE>::butterfly(acc, word_or);
                    if ((acc & want) == want) break;
                }
            }
        }
        if constexpr (CLS != VGL_RC_WAVE) acc = T::butterfly(acc, word_or);      // (a wave's is whole already)
        const ms_word nw = acc & want;
        if constexpr (CLS == VGL_RC_WG) {
            if (T::lead() && nw != 0 && atomicOr(t.nxt + v, nw) == 0) {
                const int k = t.out.cls[v];
#pragma unroll
                for (int c = 0; c < VGL_RC_N; c++)
                    if (k == c) {
                        const ms_word pos = atomicAdd(t.out.cnt + MS_TAIL + c, 1ull);
                        if (pos < (ms_word)t.out.next.cap[c]) t.out.next.rows[c][pos] = v;
                    }
            }
        } else {
            const bool app = T::lead() && nw != 0;
            if (app) t.nxt[v] = nw;
            ms_append(st, app, v, t.out);
        }
    }
    if constexpr (CLS != VGL_RC_WG) ms_flush_all(st, t.out);
    vgl_wave_flush_add(t.out.cnt + MS_PULLED, examined);
}

// ---- settle ----
struct ms_settle {
    ms_lists next, old;
    int32_t old_n[VGL_RC_N];      // the old lists' lengths (the host knows them); the next lists' are read from cnt
    ms_word *cnt;
    ms_word *seen;
    const ms_word *nxt;          // the words of the new frontier: cur from the next level on
    ms_word *old_cur;            // the words of the old frontier: cleared, nxt from the next level on
    const int64_t *rowptr;       // the traversal direction
    int32_t *levels;             // may be NULL
    int32_t V, level, base, nb;
};
__device__ __forceinline__ int32_t ms_list_at(const ms_lists &l, int64_t i, int64_t n0, int64_t n1)
{
    return i < n0 ? l.rows[0][i] : i < n0 + n1 ? l.rows[1][i - n0] : l.rows[2][i - n0 - n1];
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_msbfs_settle(ms_settle a)
{
    const int lane = vgl_lane();
    const int64_t n0 = (int64_t)min(a.cnt[MS_TAIL + 0], (ms_word)a.next.cap[0]), n1 = (int64_t)min(a.cnt[MS_TAIL + 1], (ms_word)a.next.cap[1]),
                  n2 = (int64_t)min(a.cnt[MS_TAIL + 2], (ms_word)a.next.cap[2]);
    const int64_t total = n0 + n1 + n2;
    int64_t deg = 0, bits = 0;
    ms_word mine = 0;                                                 // lane b: vertices reached for source b
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < total; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        ms_word nw = 0;
        if (i < total) {
            const int32_t v = ms_list_at(a.next, i, n0, n1);
            nw = a.nxt[v];
            a.seen[v] |= nw;
            deg += a.rowptr[v + 1] - a.rowptr[v];
            bits += __popcll(nw);
            if (a.levels)
                for (ms_word m = nw; m; m &= m - 1) a.levels[(int64_t)(a.base + (__ffsll((long long)m) - 1)) * a.V + v] = a.level;
        }
        if (__any(nw != 0))                                           // (uniform) the transpose: 64 vertices by 64 sources
            for (int b = 0; b < a.nb; b++) {
                const ms_word m = __ballot((nw >> b) & 1ull);
                if (lane == b) mine += (ms_word)__popcll(m);
            }
    }
    const int64_t o0 = a.old_n[0], o1 = a.old_n[1], ototal = o0 + o1 + a.old_n[2];
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < ototal; i += (int64_t)gridDim.x * VGL_BLOCK) a.old_cur[ms_list_at(a.old, i, o0, o1)] = 0;
    if (mine) atomicAdd(a.cnt + MS_SRC + lane, mine);
    vgl_wave_flush_add(a.cnt + MS_ENTRIES, deg);
    vgl_wave_flush_add(a.cnt + MS_BITS, bits);
}

// ---- fold and publish: one workgroup of 64 threads; d = the distance the level reached (0: after the seed, nothing to fold) ----
__global__ __launch_bounds__(MS_BATCH) void vgl_k_msbfs_publish(ms_word *cnt, int32_t nb, int32_t base, int32_t d, int64_t *reached, int64_t *dist_sum, int32_t *ecc, double *harmonic,
                                                                 volatile int64_t *host, int64_t seq)
{
    const int b = threadIdx.x;
    const ms_word c = cnt[MS_SRC + b];
    cnt[MS_SRC + b] = 0;
    if (b < nb && c > 0 && d > 0) {
        if (reached) reached[base + b] += (int64_t)c;
        if (dist_sum) dist_sum[base + b] += (int64_t)c * d;
        if (ecc) ecc[base + b] = d;
        if (harmonic) harmonic[base + b] = harmonic[base + b] + (double)(int64_t)c / (double)d;
    }
    if (b < MS_NPUB) {
        host[b] = (int64_t)cnt[b];
        cnt[b] = 0;
    }
    __threadfence_system();
    __syncthreads();
    if (b == 0) { host[C_NSLOTS] = seq; __threadfence_system(); }
}

}  // namespace

// what is per graph and not per run: per direction the class of every row, the rows by class (the pull runs over them) and the longest row, under
// the switches `key` (cached on the handle, freed with it).  bc's cached classes do not fit as they are: four classes under VGL_BC_* switches, no row lists.
struct vgl_msbfs_cache {
    struct dir_classes {
        vgl_dev<uint8_t> cls;                        // V
        vgl_dev<int32_t> rows;                       // V: the rows of class 0, then 1, then 2
        int64_t size[VGL_RC_N] = {};
        int64_t max_row = 0;
        bool ready = false;
    } dir[2];                                        // 0 = outgoing, 1 = incoming
    int64_t key[2] = {-1, -1};
    vgl_rc_bounds b{};
};

template <> void vgl_cache_free(vgl_msbfs_cache *p) { delete p; }

namespace {

int ms_classify_dir(vgl_hip_ctx *c, vgl_hip_graph *g, vgl_msbfs_cache *k, int d)
{
    hipStream_t st = c->stream;
    const vgl_dir_csr &csr = d == 0 ? g->out : g->in;
    vgl_msbfs_cache::dir_classes &dc = k->dir[d];
    const int32_t V = g->V;
    VGL_TRY(dc.cls.alloc((size_t)V));
    VGL_TRY(dc.rows.alloc((size_t)V));
    vgl_dev<ms_word> tmp;                                            // sizes (3), longest row (1), list tails (3)
    VGL_TRY(tmp.alloc(st, 8));
    VGL_HIP_TRY(hipMemsetAsync(tmp, 0, sizeof(ms_word) * 8, st));
    ms_word h[4] = {0, 0, 0, 0};
    if (V > 0) {
        hipLaunchKernelGGL(vgl_k_msbfs_classify, dim3(vgl_grid(V, VGL_BLOCK, MS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, csr.rowptr, k->b, dc.cls.p, tmp.p, tmp.p + 3);
        VGL_HIP_TRY(hipGetLastError());
        VGL_HIP_TRY(hipMemcpyAsync(h, tmp, sizeof(h), hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (h[0] + h[1] + h[2] != (ms_word)V) VGL_FAIL("msbfs_prepare: internal error (the row classes do not add up to the vertices)");
        hipLaunchKernelGGL(vgl_k_msbfs_rows, dim3(vgl_grid(V, VGL_BLOCK, MS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const uint8_t *)dc.cls.p, dc.rows.p, dc.rows.p + h[0],
                           dc.rows.p + h[0] + h[1], tmp.p + 4);
        VGL_HIP_TRY(hipGetLastError());
        VGL_HIP_TRY(hipStreamSynchronize(st));
    }
    for (int i = 0; i < VGL_RC_N; i++) dc.size[i] = (int64_t)h[i];
    dc.max_row = (int64_t)h[3];
    dc.ready = true;
    return 0;
}

// the CSRs a run reads: push = the traversal direction, pull = its reverse (-1: none, the run is push-only)
struct ms_plan { int push, pull; };

int ms_validate(const char *who, vgl_hip_ctx *c, vgl_hip_graph *g, int direction, int symmetric, ms_plan *plan)
{
    static thread_local std::string msg;
    if (!c || !g) { msg = std::string(who) + ": null argument"; VGL_FAIL(msg.c_str()); }
    if (g->row_begin != 0 || g->row_end != g->V) { msg = std::string(who) + ": graph handle must own all rows (multi-source BFS has no sharded form)"; VGL_FAIL(msg.c_str()); }
    if (direction != 0 && direction != 1) { msg = std::string(who) + ": direction must be 0 (along outgoing entries) or 1 (along incoming entries)"; VGL_FAIL(msg.c_str()); }
    const bool has_in = g->in.rowptr != nullptr;
    if (symmetric) { plan->push = 0; plan->pull = 0; }
    else if (direction == 0) { plan->push = 0; plan->pull = has_in ? 1 : -1; }
    else {
        if (!has_in) { msg = std::string(who) + ": direction 1 needs the incoming CSR, or symmetric = 1 from a caller who vouches that the stored graph is symmetric"; VGL_FAIL(msg.c_str()); }
        plan->push = 1; plan->pull = 0;
    }
    return 0;
}

// the classes of the directions `plan` reads, under the switches as they stand; *built: something was built now
int ms_ensure(vgl_hip_ctx *c, vgl_hip_graph *g, ms_plan plan, vgl_msbfs_cache **out, bool *built)
{
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_MSBFS_SHORT", "VGL_MSBFS_WAVE");
    const int64_t key[2] = {b.shrt, b.wave};
    *built = false;
    if (!g->msbfs) g->msbfs.reset(new vgl_msbfs_cache());
    vgl_msbfs_cache *k = g->msbfs.get();
    if (!std::equal(key, key + 2, k->key)) {
        VGL_HIP_TRY(hipStreamSynchronize(c->stream));               // (kernels of an earlier run may still read the classes)
        k->dir[0].ready = k->dir[1].ready = false;
        k->b = b;
        std::copy(key, key + 2, k->key);
    }
    for (int d = 0; d < 2; d++)
        if ((plan.push == d || plan.pull == d) && !k->dir[d].ready) {
            VGL_TRY(ms_classify_dir(c, g, k, d));
            *built = true;
        }
    *out = k;
    return 0;
}

enum { MS_MODE_AUTO = 0, MS_MODE_PUSH = 1, MS_MODE_PULL = 2 };
int ms_mode(vgl_hip_ctx *c, int *mode)
{
    const char *s = vgl_env(c, "VGL_MSBFS_MODE");
    if (!s || !*s || !strcmp(s, "auto")) *mode = MS_MODE_AUTO;
    else if (!strcmp(s, "push")) *mode = MS_MODE_PUSH;
    else if (!strcmp(s, "pull")) *mode = MS_MODE_PULL;
    else VGL_FAIL("msbfs_run: VGL_MSBFS_MODE must be auto, push or pull");
    return 0;
}

ms_lists ms_lists_of(int32_t *rows, const int64_t *size)
{
    ms_lists l;
    int64_t off = 0;
    for (int k = 0; k < VGL_RC_N; k++) {
        l.rows[k] = rows + off;
        l.cap[k] = (int32_t)size[k];
        off += size[k];
    }
    return l;
}

}  // namespace

extern "C" {

int vgl_hip_msbfs_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int direction, int symmetric)
{
    ms_plan plan;
    VGL_TRY(ms_validate("msbfs_prepare", c, g, direction, symmetric, &plan));
    vgl_msbfs_cache *k = nullptr;
    bool built = false;
    VGL_TRY(ms_ensure(c, g, plan, &k, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_msbfs_run(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *sources, int32_t count, int direction, int symmetric, int64_t *d_reached, int64_t *d_dist_sum,
                      int32_t *d_ecc, double *d_harmonic, int32_t *d_levels, vgl_hip_msbfs_stats *stats)
{
    // every refusal comes before the first write to an output
    ms_plan plan;
    VGL_TRY(ms_validate("msbfs_run", c, g, direction, symmetric, &plan));
    if (count < 0) VGL_FAIL("msbfs_run: count must not be negative");
    if (!d_reached && !d_dist_sum && !d_ecc && !d_harmonic && !d_levels) VGL_FAIL("msbfs_run: all outputs are NULL (give at least one of d_reached, d_dist_sum, d_ecc, d_harmonic, d_levels)");
    if (count > 0 && !sources) VGL_FAIL("msbfs_run: sources must not be NULL");
    const int32_t V = g->V;
    for (int32_t i = 0; i < count; i++)
        if (sources[i] < 0 || sources[i] >= V) VGL_FAIL("msbfs_run: source vertex out of range");
    int mode = MS_MODE_AUTO;
    VGL_TRY(ms_mode(c, &mode));
    if (mode == MS_MODE_PULL && plan.pull < 0) VGL_FAIL("msbfs_run: VGL_MSBFS_MODE=pull needs the reverse CSR of the traversal direction (the incoming CSR, or symmetric = 1)");
    const char *share_env = vgl_env(c, "VGL_MSBFS_PULL_SHARE");
    const double share = (share_env && *share_env) ? atof(share_env) : 0.05;
    const int64_t chunk_env = vgl_rc_env_chunk(c, "VGL_MSBFS_CHUNK");
    vgl_msbfs_cache *k = nullptr;
    bool built = false;
    VGL_TRY(ms_ensure(c, g, plan, &k, &built));
    hipStream_t st = c->stream;
    vgl_hip_msbfs_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    if (count == 0) {
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (stats) *stats = out;
        return 0;
    }

    const vgl_dir_csr &push_csr = plan.push == 0 ? g->out : g->in;
    const vgl_msbfs_cache::dir_classes &push_cls = k->dir[plan.push];
    const vgl_dir_csr *pull_csr = plan.pull < 0 ? nullptr : plan.pull == 0 ? &g->out : &g->in;
    const vgl_msbfs_cache::dir_classes *pull_cls = plan.pull < 0 ? nullptr : &k->dir[plan.pull];
    const int64_t E = push_csr.edges;

    // ---- scratch of the call, all of it drawn before the level loop ----
    vgl_dev<ms_word> seen, word_a, word_b, cnt;
    vgl_dev<int32_t> list_a, list_b, src;
    VGL_TRY(seen.alloc(st, (size_t)V));
    VGL_TRY(word_a.alloc(st, (size_t)V));
    VGL_TRY(word_b.alloc(st, (size_t)V));
    VGL_TRY(list_a.alloc(st, (size_t)V));
    VGL_TRY(list_b.alloc(st, (size_t)V));
    VGL_TRY(cnt.alloc(st, MS_NCNT));
    VGL_TRY(src.alloc(st, (size_t)count));
    VGL_HIP_TRY(hipMemcpyAsync(src, sources, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, st));
    VGL_HIP_TRY(hipStreamSynchronize(st));                            // (the caller's array is free again)
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(ms_word) * MS_NCNT, st));
    if (d_levels) VGL_HIP_TRY(hipMemsetAsync(d_levels, 0xFF, sizeof(int32_t) * (size_t)count * (size_t)V, st));      // -1: unreached
    const vgl_rc_chunks push_ch = vgl_rc_chunks::of(chunk_env, push_cls.max_row), pull_ch = vgl_rc_chunks::of(chunk_env, pull_cls ? pull_cls->max_row : 0);
    const ms_lists pull_rows = pull_cls ? ms_lists_of(pull_cls->rows.p, pull_cls->size) : ms_lists{};
    const int64_t grid_cap[VGL_RC_N] = {MS_MAX_GRID, MS_MAX_GRID, 4 * MS_MAX_GRID};
    auto publish = [&](int32_t nb, int32_t base, int32_t d) -> int {
        const int64_t seq = vgl_next_seq(c);
        {
            vgl_timed_launch tl(c, "msbfs_publish");
            hipLaunchKernelGGL(vgl_k_msbfs_publish, dim3(1), dim3(MS_BATCH), 0, st, cnt.p, nb, base, d, d_reached, d_dist_sum, d_ecc, d_harmonic, (volatile int64_t *)c->h_counters, seq);
        }
        VGL_HIP_TRY(hipGetLastError());
        return vgl_wait_counters(c, seq);
    };

    const char *const push_slot[VGL_RC_N] = {"msbfs_push_short", "msbfs_push_wave", "msbfs_push_wg"};
    const char *const pull_slot[VGL_RC_N] = {"msbfs_pull_short", "msbfs_pull_wave", "msbfs_pull_wg"};
    int64_t words_total = 0;                                          // (vertex, level) pairs: the lengths of all frontiers
    for (int32_t base = 0; base < count; base += MS_BATCH) {
        const int32_t nb = std::min<int32_t>(MS_BATCH, count - base);
        const ms_word active = nb == MS_BATCH ? ~0ull : (1ull << nb) - 1ull;
        ms_word *cur = word_a, *nxt = word_b;
        ms_lists now = ms_lists_of(list_a, push_cls.size), next = ms_lists_of(list_b, push_cls.size);
        VGL_HIP_TRY(hipMemsetAsync(seen, 0, sizeof(ms_word) * (size_t)V, st));
        VGL_HIP_TRY(hipMemsetAsync(word_a, 0, sizeof(ms_word) * (size_t)V, st));
        VGL_HIP_TRY(hipMemsetAsync(word_b, 0, sizeof(ms_word) * (size_t)V, st));
        hipLaunchKernelGGL(vgl_k_msbfs_seed, dim3(1), dim3(MS_BATCH), 0, st, (const int32_t *)src.p, nb, base, V, push_csr.rowptr, cur, seen.p, now, (const uint8_t *)push_cls.cls.p, cnt.p,
                           d_reached, d_dist_sum, d_ecc, d_harmonic, d_levels);
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(publish(nb, base, 0));
        int64_t n[VGL_RC_N], entries = c->h_counters[MS_ENTRIES];
        for (int i = 0; i < VGL_RC_N; i++) n[i] = c->h_counters[MS_TAIL + i];
        out.reached_total += nb;
        int32_t expanded = 0;
        for (int32_t d = 1;; d++) {                                   // the frontier at distance d - 1 is expanded
            const int64_t total = n[0] + n[1] + n[2];
            for (int i = 0; i < VGL_RC_N; i++)
                if (n[i] < 0 || n[i] > now.cap[i]) VGL_FAIL("msbfs_run: internal error (a frontier list longer than its row class)");
            if (total == 0) break;
            if (d > V) VGL_FAIL("msbfs_run: internal error (more levels than vertices)");
            words_total += total;
            const bool pull = mode == MS_MODE_PULL || (mode == MS_MODE_AUTO && pull_csr && (double)entries > share * (double)E);
            ms_level t;
            t.cur = cur; t.seen = seen; t.nxt = nxt; t.active = active;
            t.out.next = next; t.out.cls = push_cls.cls; t.out.cnt = cnt;
            const ms_lists &from = pull ? pull_rows : now;
            const int32_t *const rows[VGL_RC_N] = {from.rows[0], from.rows[1], from.rows[2]};
            if (!pull) {
                t.rowptr = push_csr.rowptr; t.adj = push_csr.adj; t.ch = push_ch;
                VGL_TRY(vgl_rc_launch_trio(c, push_slot, n, grid_cap, t.ch, vgl_k_msbfs_push<VGL_RC_SHORT>, vgl_k_msbfs_push<VGL_RC_WAVE>, vgl_k_msbfs_push<VGL_RC_WG>, rows, t));
                out.levels_push++;
                out.edges_push += entries;
            } else {
                t.rowptr = pull_csr->rowptr; t.adj = pull_csr->adj; t.ch = pull_ch;
                VGL_TRY(vgl_rc_launch_trio(c, pull_slot, pull_cls->size, grid_cap, t.ch, vgl_k_msbfs_pull<VGL_RC_SHORT>, vgl_k_msbfs_pull<VGL_RC_WAVE>, vgl_k_msbfs_pull<VGL_RC_WG>, rows, t));
                out.levels_pull++;
            }
            {
                ms_settle a;
                a.next = next; a.old = now;
                for (int i = 0; i < VGL_RC_N; i++) a.old_n[i] = (int32_t)n[i];
                a.cnt = cnt; a.seen = seen; a.nxt = nxt; a.old_cur = cur; a.rowptr = push_csr.rowptr; a.levels = d_levels;
                a.V = V; a.level = d + 1; a.base = base; a.nb = nb;
                // the next frontier has at most one vertex per entry of this one (push) or V (pull)
                const int64_t bound = std::max(total, pull ? (int64_t)V : std::min<int64_t>(V, entries));
                vgl_timed_launch tl(c, "msbfs_settle");
                hipLaunchKernelGGL(vgl_k_msbfs_settle, dim3(vgl_grid(bound, VGL_BLOCK, MS_MAX_GRID)), dim3(VGL_BLOCK), 0, st, a);
            }
            VGL_HIP_TRY(hipGetLastError());
            VGL_TRY(publish(nb, base, d));
            expanded++;
            for (int i = 0; i < VGL_RC_N; i++) n[i] = c->h_counters[MS_TAIL + i];
            entries = c->h_counters[MS_ENTRIES];
            out.reached_total += c->h_counters[MS_BITS];
            out.edges_pull += c->h_counters[MS_PULLED];
            std::swap(cur, nxt);
            std::swap(now, next);
        }
        out.batches++;
        out.sources += nb;
        out.levels_total += expanded;
        out.max_depth = std::max(out.max_depth, expanded - 1);
    }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    // the model: per batch the three word arrays cleared; per entry walked the adjacency entry and one 8-byte word of its far
    // end; per pull level the row list and the seen word of every vertex; per frontier vertex its list entry written and read twice, its words
    // (nxt read, seen read and written, cur cleared), its row bounds in the level and in settle; the levels rows when asked for
    out.algorithmic_bytes = 24 * (int64_t)V * out.batches + 12 * (out.edges_push + out.edges_pull) + 12 * (int64_t)V * out.levels_pull + 76 * words_total +
                            (d_levels ? 4 * (int64_t)count * V + 4 * out.reached_total : 0);
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
