// vgl_rowclass.h -- the short / wave / workgroup row-class layer of the worklist algorithms (kcore, ktruss, msf, msbfs, bicc, mis, sim, subgraph).
// DESIGN section 21.  A row (or an edge's shorter row) falls into one of three classes by its length; items are appended to one list per class; the
// host keeps a [head, tail) window per list, read from the pinned counter mirror, and every step launches one kernel per class that has items.
// Here: the bounds, the windows, the per-class launch, the append staging, the class-list builder (count, check, carve, fill) and the team: what a
// kernel that serves all three classes from one body needs of its class.  bc (four classes), tri and lp (plan-owned sorted lists) are other schemes.
// Not on the team, because their three forms are three structures: kcore_short / wave (no grid stride, early return) and kcore_wg (2-D grid);
// msf_min_* (offer combining in the short form).  Chunked workgroup rows (vgl_chunks.h) are the team's workgroup items in msbfs_push / pull.  Not on the builder:
// vgl_k_sub_classify / _lists (two directions and old_id in one pass), vgl_k_bicc_init / _seed (union-find and level set-up in the same pass),
// ktruss / kcore / msbfs (vgl_wave_append lists that grow during the run).
#pragma once
#include "vgl_hip_internal.h"
#include "vgl_chunks.h"

// ---- classes and bounds ----
constexpr int VGL_RC_N = 3;
enum { VGL_RC_SHORT = 0, VGL_RC_WAVE = 1, VGL_RC_WG = 2 };
constexpr int VGL_RC_G = 8;                      // lanes per short row
struct vgl_rc_bounds { int32_t shrt, wave; };
__host__ __device__ inline int vgl_rc_class_of(int64_t d, vgl_rc_bounds b) { return d <= b.shrt ? VGL_RC_SHORT : d <= b.wave ? VGL_RC_WAVE : VGL_RC_WG; }
// the bounds as the two environment switches of the algorithm give them: 32 and 1024 unless set, 0 <= short <= 2^20, short <= wave <= 2^24
static inline vgl_rc_bounds vgl_rc_env_bounds(vgl_hip_ctx *c, const char *env_short, const char *env_wave)
{
    vgl_rc_bounds b;
    b.shrt = (int32_t)vgl_env_int(c, env_short, 32, 0, 1 << 20);
    b.wave = (int32_t)vgl_env_int(c, env_wave, 1024, b.shrt, 1 << 24);
    return b;
}

// ---- host windows: list k holds the current items in [head[k], tail[k]); the tails are cumulative device counters ----
struct vgl_rc_window {
    int64_t head[VGL_RC_N] = {0, 0, 0}, tail[VGL_RC_N] = {0, 0, 0};
    int64_t n(int k) const { return tail[k] - head[k]; }
    int64_t live() const { return n(0) + n(1) + n(2); }                 // items of the current step
    int64_t total() const { return tail[0] + tail[1] + tail[2]; }       // items appended so far
    // the step is done: head moves to tail and the new tails are read (the pinned mirror's slots); `what` is the caller's error for a list
    // whose tail went backwards or past its capacity
    int advance(const int64_t *tails, const int64_t *cap, const char *what)
    {
        for (int k = 0; k < VGL_RC_N; k++) {
            head[k] = tail[k];
            tail[k] = tails[k];
            if (tail[k] < head[k] || tail[k] > cap[k]) VGL_FAIL(what);
        }
        return 0;
    }
    int advance(const int64_t *tails, int64_t cap, const char *what)
    {
        const int64_t caps[VGL_RC_N] = {cap, cap, cap};
        return advance(tails, caps, what);
    }
};

// ---- per-class launch: for every class with items, launch(k, n[k]) under the timing slot slot[k]; then the one error check of the step ----
template <class F>
static inline int vgl_rc_launch(vgl_hip_ctx *c, const char *const *slot, const int64_t *n, F &&launch)
{
    for (int k = 0; k < VGL_RC_N; k++)
        if (n[k] > 0) {
            vgl_timed_launch tl(c, slot[k]);
            launch(k, n[k]);
        }
    VGL_HIP_TRY(hipGetLastError());
    return 0;
}
template <class F>
static inline int vgl_rc_launch(vgl_hip_ctx *c, const char *const *slot, const vgl_rc_window &w, F &&launch)
{
    const int64_t n[VGL_RC_N] = {w.n(0), w.n(1), w.n(2)};
    return vgl_rc_launch(c, slot, n, launch);
}
// the three instantiations of a team kernel `k<CLS>(LIST list, int32_t n, args...)`: class k runs over list[k] under slot[k], on at most cap[k] workgroups.
// A kernel whose workgroup rows are chunked by `wg` (it finds the chunks among its args) has wg.nchunks workgroup items per row.
template <class LIST, class... KA, class... A>
static inline int vgl_rc_launch_trio(vgl_hip_ctx *c, const char *const *slot, const int64_t *n, const int64_t *cap, vgl_rc_chunks wg, void (*k_short)(LIST, int32_t, KA...),
                                     void (*k_wave)(LIST, int32_t, KA...), void (*k_wg)(LIST, int32_t, KA...), const LIST *list, const A &...args)
{
    void (*const k[VGL_RC_N])(LIST, int32_t, KA...) = {k_short, k_wave, k_wg};
    const int64_t items_per_wg[VGL_RC_N] = {VGL_BLOCK / VGL_RC_G, VGL_WAVES, 1}, items_per_row[VGL_RC_N] = {1, 1, wg.nchunks};
    return vgl_rc_launch(c, slot, n, [&](int cls, int64_t m) {
        hipLaunchKernelGGL(k[cls], dim3(vgl_grid(m * items_per_row[cls], items_per_wg[cls], cap[cls])), dim3(VGL_BLOCK), 0, c->stream, list[cls], (int32_t)m, args...);
    });
}
template <class LIST, class... KA, class... A>
static inline int vgl_rc_launch_trio(vgl_hip_ctx *c, const char *const *slot, const int64_t *n, const int64_t *cap, void (*k_short)(LIST, int32_t, KA...),
                                     void (*k_wave)(LIST, int32_t, KA...), void (*k_wg)(LIST, int32_t, KA...), const LIST *list, const A &...args)
{
    return vgl_rc_launch_trio(c, slot, n, cap, vgl_rc_chunks::whole(), k_short, k_wave, k_wg, list, args...);
}
template <class LIST, class... KA, class... A>
static inline int vgl_rc_launch_trio(vgl_hip_ctx *c, const char *const *slot, const vgl_rc_window &w, const int64_t *cap, void (*k_short)(LIST, int32_t, KA...),
                                     void (*k_wave)(LIST, int32_t, KA...), void (*k_wg)(LIST, int32_t, KA...), const LIST *list, const A &...args)
{
    const int64_t n[VGL_RC_N] = {w.n(0), w.n(1), w.n(2)};
    return vgl_rc_launch_trio(c, slot, n, cap, k_short, k_wave, k_wg, list, args...);
}

#ifdef __HIPCC__
// ---- append staging: a wave collects its appends in LDS and takes one returning atomic per 64 or more of them ----
constexpr int VGL_RC_STAGE = 128;                // LDS slots per wave and class (fewer than 64 wait, at most 64 arrive)
// where a position of the cumulative tail lands: on a ring (msf: a round reads [head, tail) and appends behind tail) or in a list that drops what
// runs past its end (msbfs: the host refuses the level)
struct vgl_rc_ring {
    int32_t *rows; uint32_t cap;
    __device__ __forceinline__ void put(unsigned long long pos, int32_t v) const { rows[pos % cap] = v; }
};
struct vgl_rc_bounded {
    int32_t *rows; int32_t cap;
    __device__ __forceinline__ void put(unsigned long long pos, int32_t v) const { if (pos < (unsigned long long)cap) rows[pos] = v; }
};
// `n` (uniform over the wave) items wait in `buf` (LDS, VGL_RC_STAGE slots, this wave's own); every lane of the wave calls keep and flush
struct vgl_rc_stage {
    int32_t *buf; int n;
    template <class LIST> __device__ __forceinline__ void flush(const LIST &to, unsigned long long *tail)
    {
        if (n == 0) return;                                           // (uniform)
        unsigned long long base = 0;
        if (vgl_lane() == 0) base = atomicAdd(tail, (unsigned long long)n);
        base = __shfl(base, 0);
        for (int j = vgl_lane(); j < n; j += 64) to.put(base + (unsigned long long)j, buf[j]);
        __builtin_amdgcn_wave_barrier();
        n = 0;
    }
    template <class LIST> __device__ __forceinline__ void keep(bool want, int32_t v, const LIST &to, unsigned long long *tail)
    {
        const unsigned long long m = __ballot(want);
        if (!m) return;                                               // (uniform)
        if (want) buf[n + __popcll(m & ((1ull << vgl_lane()) - 1ull))] = v;
        n += __popcll(m);
        __builtin_amdgcn_wave_barrier();
        if (n >= 64) flush(to, tail);
    }
};
// the NST empty stages of this wave, in the workgroup's LDS (NST * VGL_WAVES * VGL_RC_STAGE ints); once per kernel
template <int NST>
__device__ __forceinline__ void vgl_rc_stage_open(vgl_rc_stage (&st)[NST])
{
    __shared__ int32_t s_keep[NST][VGL_WAVES][VGL_RC_STAGE];
#pragma unroll
    for (int c = 0; c < NST; c++) st[c] = vgl_rc_stage{s_keep[c][vgl_wave()], 0};
}

// ---- the team: the lanes that share an item in the kernel of class CLS (8 of a wave, a wave, the workgroup) ----
// The item loop is   for (int64_t at = T::begin(); at < n; at += T::stride()) { const int64_t i = T::item(at); const bool has = i < n; ... }
// Short: `at` is the workgroup's first item, so every lane of the workgroup makes the same trips, and a lane whose team has no item (has == false)
// walks an empty row: barriers, ballots and staged appends in the body see whole waves.  Wave: uniform over the wave.  Workgroup: uniform over the
// workgroup.  There i == at and `has` is always true.
// The reductions and rank() are called by every lane of the team's wave(s) in uniform control flow; each workgroup form keeps its LDS itself.
template <int CLS>
struct vgl_rc_team {
    static constexpr int LANES = CLS == VGL_RC_SHORT ? VGL_RC_G : CLS == VGL_RC_WAVE ? 64 : VGL_BLOCK;
    static constexpr int ITEMS_PER_WG = VGL_BLOCK / LANES;
    static __device__ __forceinline__ int lane() { return CLS == VGL_RC_WG ? threadIdx.x : threadIdx.x & (LANES - 1); }
    static __device__ __forceinline__ bool lead() { return lane() == 0; }
    static __device__ __forceinline__ int team() { return CLS == VGL_RC_WG ? 0 : threadIdx.x / LANES; }      // of the workgroup's
    static __device__ __forceinline__ int64_t begin() { return (int64_t)blockIdx.x * ITEMS_PER_WG + (CLS == VGL_RC_SHORT ? 0 : team()); }
    static __device__ __forceinline__ int64_t stride() { return (int64_t)gridDim.x * ITEMS_PER_WG; }
    static __device__ __forceinline__ int64_t item(int64_t at) { return at + (CLS == VGL_RC_SHORT ? team() : 0); }
    // a loop condition over the team's row that keeps the wave together: the eight teams of a short wave leave with the longest of their rows
    static __device__ __forceinline__ bool together(bool go_on) { return CLS == VGL_RC_SHORT ? __any(go_on) : go_on; }
    // Chunked workgroup rows: the workgroup form's items are the (row, piece) pairs of `ch`, the other forms' the rows of the list.  The item loop
    // runs to items(n, ch); item i is piece k = piece(i, ch, &row) of list entry `row`; range() is that piece of the row [row_lo, row_end), false
    // when it is empty (then *lo == *hi).  Short and wave: statically the whole row, `ch` is not read.
    static __device__ __forceinline__ int64_t items(int32_t n, const vgl_rc_chunks &ch) { if constexpr (CLS == VGL_RC_WG) return (int64_t)n * ch.nchunks; else return n; }
    static __device__ __forceinline__ int64_t piece(int64_t i, const vgl_rc_chunks &ch, int64_t *row)
    {
        int64_t k = 0;
        if constexpr (CLS == VGL_RC_WG) ch.split(i, row, &k);
        else *row = i;
        return k;
    }
    static __device__ __forceinline__ bool range(const vgl_rc_chunks &ch, int64_t row_lo, int64_t row_end, int64_t k, int64_t *lo, int64_t *hi)
    {
        if constexpr (CLS == VGL_RC_WG) {
            if (ch.range(row_lo, row_end, k, lo, hi)) return true;
            *hi = *lo;
            return false;
        } else { *lo = row_lo; *hi = row_end; return true; }
    }

    // the combine of v over the team by OP, in every lane: an xor-butterfly over the team's lanes of a wave; the workgroup then folds the four
    // waves' results from LDS in wave order
    template <class T, class OP>
    static __device__ __forceinline__ T butterfly(T v, OP op)
    {
#pragma unroll
        for (int o = (LANES < 64 ? LANES : 64) / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
        if constexpr (CLS == VGL_RC_WG) {
            __shared__ T s_red[VGL_WAVES];
            __syncthreads();                                          // the results of the item before have been read
            if (vgl_lane() == 0) s_red[vgl_wave()] = v;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < VGL_WAVES; w++) v = op(v, s_red[w]);
        }
        return v;
    }
    template <class T> static __device__ __forceinline__ T min_of(T v) { return butterfly(v, [](T a, T b) { return a < b ? a : b; }); }
    template <class T> static __device__ __forceinline__ T max_of(T v) { return butterfly(v, [](T a, T b) { return a > b ? a : b; }); }
    // the sum: the workgroup's is 0 + wave 0 + wave 1 + wave 2 + wave 3 (a floating-point sum keeps this shape)
    template <class T>
    static __device__ __forceinline__ T sum_of(T v)
    {
        if constexpr (CLS == VGL_RC_WG) {
            __shared__ T s_sum[VGL_WAVES];
            return vgl_block_reduce_add(v, s_sum);
        } else return butterfly(v, [](T a, T b) { return a + b; });
    }
    // the bitwise or of the low `nbits` bits
    static __device__ __forceinline__ int or_of(int bits, int nbits)
    {
        if constexpr (CLS == VGL_RC_SHORT) return butterfly(bits, [](int a, int b) { return a | b; });
        else {
            int all = 0;
#pragma unroll
            for (int b = 0; b < nbits; b++) all |= __any(bits & (1 << b)) ? 1 << b : 0;
            if constexpr (CLS == VGL_RC_WG) {
                __shared__ int s_bits;
                if (threadIdx.x == 0) s_bits = 0;
                __syncthreads();
                if (vgl_lane() == 0 && all) atomicOr(&s_bits, all);
                __syncthreads();
                all = s_bits;
                __syncthreads();                                      // read before the next item clears it
            }
            return all;
        }
    }
    // the ordered rank of a predicate: how many lanes of the team below this one hold k; *total = how many of the team do
    static __device__ __forceinline__ int rank(bool k, int *total)
    {
        const unsigned long long m = __ballot(k);
        if constexpr (CLS == VGL_RC_SHORT) {
            const unsigned sub = (unsigned)(m >> (vgl_lane() & ~(LANES - 1))) & ((1u << LANES) - 1u);      // the team's 8 bits of the 64-bit ballot
            *total = __popc(sub);
            return __popc(sub & ((1u << lane()) - 1u));
        } else {
            int pre = 0, tot = __popcll(m);
            if constexpr (CLS == VGL_RC_WG) {
                __shared__ int s_cnt[VGL_WAVES];
                __syncthreads();                                      // the counts of the chunk before have been read
                if (vgl_lane() == 0) s_cnt[vgl_wave()] = tot;
                __syncthreads();
                tot = 0;
#pragma unroll
                for (int w = 0; w < VGL_WAVES; w++) {
                    const int x = s_cnt[w];
                    if (w < vgl_wave()) pre += x;
                    tot += x;
                }
            }
            *total = tot;
            return pre + __popcll(m & ((1ull << vgl_lane()) - 1ull));
        }
    }
};

// ---- the class-list builder: items 0 .. n - 1 of a source S into one list per class ----
// S::cls(i, work) = the class of item i and its work, or -1 for "not an item"; it may store what the algorithm wants of the item on the way
template <class S>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_rc_count(S s, int64_t n, unsigned long long *rows, unsigned long long *bad, unsigned long long *work)
{
    int64_t r[VGL_RC_N] = {0, 0, 0}, b = 0, w = 0;
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) {
        int64_t x = 0;
        const int c = s.cls(i, x);
        if (c < 0) b++;
        else { r[c]++; w += x; }
    }
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) vgl_wave_flush_add(rows + c, r[c]);
    if (bad) vgl_wave_flush_add(bad, b);
    if (work) vgl_wave_flush_add(work, w);
}
template <class S, class LIST>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_rc_fill(S s, int64_t n, LIST L0, LIST L1, LIST L2, unsigned long long *tail)
{
    const LIST L[VGL_RC_N] = {L0, L1, L2};
    vgl_rc_stage st[VGL_RC_N];
    vgl_rc_stage_open(st);
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < n; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        int64_t x = 0;
        const int cls = i < n ? s.cls(i, x) : -1;
#pragma unroll
        for (int c = 0; c < VGL_RC_N; c++) st[c].keep(cls == c, (int32_t)i, L[c], tail + c);
    }
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) st[c].flush(L[c], tail + c);
}
// the lists of a run (LIST: vgl_rc_ring or vgl_rc_bounded): count() finds rows[], fill() carves a block into l[] and appends the items
template <class LIST>
struct vgl_rc_lists {
    vgl_dev<int32_t> mem;                        // the block, unless the caller gives its own to fill()
    LIST l[VGL_RC_N];
    int64_t rows[VGL_RC_N] = {0, 0, 0};
    // One launch under `slot` (none for n == 0; untimed for nullptr) and one publish of the `ncnt` counters: rows[] from cnt[rows0 ..]; cnt[bad0]
    // items that are none (bad_msg) and cnt[work0] the work, where the index is >= 0; the classes must add up to `expect` where that is >= 0 (sum_msg).
    template <class S>
    int count(vgl_hip_ctx *c, const char *slot, const char *publish, const S &src, int64_t n, int64_t max_grid, unsigned long long *cnt, int ncnt, int rows0, int bad0, int work0,
              int64_t expect, const char *bad_msg, const char *sum_msg)
    {
        if (n > 0) {
            {
                vgl_timed_launch tl(c, slot);
                hipLaunchKernelGGL(vgl_k_rc_count<S>, dim3(vgl_grid(n, VGL_BLOCK, max_grid)), dim3(VGL_BLOCK), 0, c->stream, src, n, cnt + rows0, bad0 < 0 ? nullptr : cnt + bad0,
                                   work0 < 0 ? nullptr : cnt + work0);
            }
            VGL_HIP_TRY(hipGetLastError());
        }
        VGL_TRY(vgl_publish_counters(c, publish, cnt, ncnt));
        if (bad0 >= 0 && c->h_counters[bad0] != 0) VGL_FAIL(bad_msg);
        int64_t total = 0;
        for (int k = 0; k < VGL_RC_N; k++) {
            rows[k] = c->h_counters[rows0 + k];
            if (rows[k] < 0) VGL_FAIL(sum_msg);
            total += rows[k];
        }
        if (expect >= 0 && total != expect) VGL_FAIL(sum_msg);
        return 0;
    }
    // One launch under `slot`: list k gets factor * rows[k] entries of `block` (nullptr: of mem, drawn here) and the items of class k; tail: its 3 counters
    template <class S>
    int fill(vgl_hip_ctx *c, const char *slot, const S &src, int64_t n, int64_t max_grid, int factor, int32_t *block, unsigned long long *tail)
    {
        if (!block) {
            VGL_TRY(mem.alloc(c->stream, (size_t)(factor * (rows[0] + rows[1] + rows[2]))));
            block = mem.p;
        }
        for (int k = 0; k < VGL_RC_N; k++) {
            l[k] = LIST{block, (decltype(LIST::cap))(factor * rows[k])};
            block += factor * rows[k];
        }
        {
            vgl_timed_launch tl(c, slot);
            hipLaunchKernelGGL((vgl_k_rc_fill<S, LIST>), dim3(vgl_grid(n, VGL_BLOCK, max_grid)), dim3(VGL_BLOCK), 0, c->stream, src, n, l[0], l[1], l[2], tail);
        }
        VGL_HIP_TRY(hipGetLastError());
        return 0;
    }
};
#endif
