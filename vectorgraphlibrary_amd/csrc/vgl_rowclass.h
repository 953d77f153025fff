// vgl_rowclass.h -- the short / wave / workgroup row-class layer of the worklist algorithms (kcore, ktruss, msf, msbfs, bicc).  DESIGN section 21.
// A row (or an edge's shorter row) falls into one of three classes by its length; items are appended to one list per class; the host keeps a
// [head, tail) window per list, read from the pinned counter mirror, and every step launches one kernel per class that has items.  What is here is
// what the five files share; their kernels, grids and counters are their own.  bc (four classes), tri and lp (plan-owned sorted lists) are other schemes.
#pragma once
#include "vgl_hip_internal.h"

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
#endif
