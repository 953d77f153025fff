// lp.hip -- label propagation (LabelPropagation::gpu_lp with the AlwaysActive condition, algorithms/lp/gpu/lp_gpu.cu:185-420,
// active_conditions.cuh:6-37): every iteration each vertex takes the most frequent label among its neighbours (ties: the largest label),
// synchronously, until an iteration changes nothing or max_iterations is reached.  The contract is written out in include/vgl_hip.h.
//
// The reference sorts every neighbourhood segment and reduces runs; here the mode is counted in a hash table per row and reduced with one
// unsigned max over packed keys  key = count << 32 | (label ^ 0x80000000):  the highest count wins first, the largest signed label second,
// and a max is exact whatever the order in which lanes, workgroups or atomics meet.  A slot whose count is 0 is empty, so every int32
// label can be stored (no sentinel label).
//
// Rows are split once per graph and direction into degree classes (vgl_lp_cache, cached on the graph handle):
//   light  (deg <= VGL_LP_LIGHT, <= 64)  : a group of 4 / 8 / 16 / 32 / 64 lanes per row, one neighbour per lane, counts by rotating the
//                                          labels through the group (__shfl), group max of the key.  No LDS.
//   table64 (deg <= VGL_LP_WAVE, <= 512) : one 64-thread workgroup per row, LDS table of pow2 >= 2 deg slots (<= 1024: 8 KiB)
//   table1k (deg <= VGL_LP_MEDIUM, <= 4096) : one 1024-thread workgroup per row, LDS table of <= 8192 slots (64 KiB: two workgroups per CU)
//   hubs   (deg > VGL_LP_MEDIUM)          : chunks of VGL_LP_HUB_CHUNK edges per workgroup, counted in LDS first and flushed into a global
//                                          table of pow2 >= 2 deg slots per hub (CAS + add), then one workgroup per 8192 slots takes the
//                                          table's max into a 64-bit atomicMax per hub and clears the slots it read.  The tables come from
//                                          one block capped at VGL_LP_HUB_SCRATCH_KB; the hubs run in batches that fit.
// Compute passes write next[v] and a bit of `changed`; the apply pass copies the changed labels afterwards (never in place).
// Frontier mode: a row none of whose neighbours changed keeps its label, so iteration t+1 evaluates only the rows reached by pushing the
// changed vertices over the REVERSE adjacency (an active bitmap), compacted and sorted into the same classes.
#include "vgl_hip_internal.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr int LP_NCLS = 8;              // light G = 4, 8, 16, 32, 64 | table64 | table1k | hubs
constexpr int LP_HUB = 7;
constexpr int LP_T64_SLOTS = 1024, LP_T1K_SLOTS = 8192;
constexpr int LP_WIDE = 1024;           // threads of the workgroups with the 64 KiB table (two per CU: 32 waves)
constexpr int LP_RCHUNK = 8192;         // global table slots per workgroup of the hub reduction
constexpr int LP_PUSH_CHUNK = 4096;     // reverse edges per workgroup of the push over large rows
constexpr int LP_MAX_GRID = 4096;

// counters of one iteration (one device-to-host copy after the compute passes)
enum { LP_CHANGED = 0, LP_PUSHED = 1, LP_ACT_ROWS = 2, LP_ACT_EDGES = 3, LP_NCNT = 4 };

struct lp_bounds { int light, wave, medium; };

__host__ __device__ inline int lp_class_of(int64_t d, lp_bounds b)
{
    if (d <= 0) return -1;
    if (d <= b.light) return d <= 4 ? 0 : d <= 8 ? 1 : d <= 16 ? 2 : d <= 32 ? 3 : 4;
    if (d <= b.wave) return 5;
    if (d <= b.medium) return 6;
    return LP_HUB;
}

__device__ __forceinline__ uint64_t lp_key(uint32_t count, int32_t label) { return (uint64_t)count << 32 | ((uint32_t)label ^ 0x80000000u); }
__device__ __forceinline__ int32_t lp_key_label(uint64_t key) { return (int32_t)((uint32_t)key ^ 0x80000000u); }
__device__ __forceinline__ uint32_t lp_hash(int32_t label, int bits) { return bits ? ((uint32_t)label * 0x9E3779B1u) >> (32 - bits) : 0u; }
__host__ __device__ inline int lp_table_bits(int64_t deg, int max_bits)    // log2 of the pow2 >= 2 deg, at least 64 slots
{
    int b = 6;
    while (b < max_bits && ((int64_t)1 << b) < 2 * deg) b++;
    return b;
}

// count `cnt` occurrences of `label` in an open-addressing table (linear probing); scope: workgroup (LDS) or agent (global)
template <int SCOPE>
__device__ __forceinline__ void lp_insert(unsigned long long *tab, int bits, int32_t label, uint32_t cnt)
{
    const unsigned long long low = (uint32_t)label ^ 0x80000000u, add = (unsigned long long)cnt << 32;
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t h = lp_hash(label, bits);
    for (;;) {
        // LDS: look before claiming; global: claim at once (one round trip to L2 instead of two)
        unsigned long long cur = SCOPE == __HIP_MEMORY_SCOPE_WORKGROUP ? __hip_atomic_load(tab + h, __ATOMIC_RELAXED, SCOPE) : 0ull;
        if (cur == 0) {
            cur = atomicCAS(tab + h, 0ull, add | low);
            if (cur == 0) return;
        }
        if ((uint32_t)cur == (uint32_t)low) { atomicAdd(tab + h, add); return; }
        h = (h + 1) & mask;
    }
}

// where the results of a compute pass go
struct lp_io {
    const int32_t *labels;
    int32_t *next;
    uint64_t *changed;          // bitmap
    const int64_t *rev_rowptr;  // reverse CSR (edges a change pushes), nullptr when there is none
    int64_t *cnt;               // LP_NCNT counters
};
struct lp_acc {
    int64_t changed = 0, pushed = 0;
    __device__ __forceinline__ void decide(const lp_io &io, int32_t v, uint64_t key)
    {
        const int32_t lab = lp_key_label(key);
        if (lab != io.labels[v]) {
            io.next[v] = lab;
            atomicOr(reinterpret_cast<unsigned long long *>(io.changed) + (v >> 6), 1ull << (v & 63));
            changed++;
            if (io.rev_rowptr) pushed += io.rev_rowptr[v + 1] - io.rev_rowptr[v];
        }
    }
    // every lane of the wave calls this once, at the end of the kernel: one atomic per wave and counter
    __device__ __forceinline__ void flush(const lp_io &io)
    {
        const int64_t c = vgl_wave_reduce_add(changed), p = vgl_wave_reduce_add(pushed);
        if (vgl_lane() == 0 && c) {
            atomicAdd(reinterpret_cast<unsigned long long *>(io.cnt + LP_CHANGED), (unsigned long long)c);
            atomicAdd(reinterpret_cast<unsigned long long *>(io.cnt + LP_PUSHED), (unsigned long long)p);
        }
    }
};

__device__ __forceinline__ bool lp_bit(const uint64_t *bits, int32_t v) { return (bits[v >> 6] >> (v & 63)) & 1ull; }

// ---- light rows: G lanes per row ----
template <int G>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_light(const int32_t *rows, const int32_t *n_rows, const int64_t *rowptr, const int32_t *adj, lp_io io)
{
    constexpr int RPB = VGL_BLOCK / G;                       // rows per workgroup and round
    const int32_t n = *n_rows;
    const int gi = threadIdx.x & (G - 1);
    lp_acc acc;
    for (int64_t base = (int64_t)blockIdx.x * RPB; base < n; base += (int64_t)gridDim.x * RPB) {      // (uniform over the workgroup)
        const int64_t r = base + threadIdx.x / G;
        int32_t v = 0;
        int deg = 0;
        int64_t s = 0;
        if (r < n) {
            v = rows[r];
            s = rowptr[v];
            deg = (int)(rowptr[v + 1] - s);
        }
        const int32_t lab = gi < deg ? io.labels[adj[s + gi]] : 0;
        // rotate the group's labels past every lane (ds_bpermute); the lane number goes through an empty asm so that the G - 1 source
        // addresses are computed per row instead of being hoisted out of the row loop into G - 1 registers
        int lane = vgl_lane();
        asm volatile("" : "+v"(lane));
        const int me = lane & (G - 1), grp = lane & ~(G - 1);
        uint32_t cnt = 1;
#pragma unroll
        for (int k = 1; k < G; k++) {
            const int src = (me + k) & (G - 1);
            const int32_t o = __builtin_amdgcn_ds_bpermute((grp + src) << 2, lab);
            cnt += (src < deg && o == lab) ? 1u : 0u;
        }
        uint64_t key = gi < deg ? lp_key(cnt, lab) : 0ull;
#pragma unroll
        for (int m = G / 2; m > 0; m >>= 1) key = max(key, (uint64_t)__shfl_xor((unsigned long long)key, m, G));
        if (gi == 0 && deg > 0) acc.decide(io, v, key);
    }
    acc.flush(io);
}

// block max of a key (all threads call; the result is valid in thread 0)
template <int THREADS>
__device__ __forceinline__ uint64_t lp_block_max(uint64_t key, unsigned long long *s_red)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) key = max(key, (uint64_t)__shfl_xor((unsigned long long)key, m));
    if (THREADS == 64) return key;
    if (vgl_lane() == 0) s_red[vgl_wave()] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < THREADS / 64; w++) key = max(key, (uint64_t)s_red[w]);
    return key;
}

// count the labels of adj[s, s + len) into the LDS table (cleared by the caller); 4 loads in flight per thread
template <int THREADS>
__device__ __forceinline__ void lp_count_lds(unsigned long long *tab, int bits, const int32_t *adj, int64_t s, int64_t len, const int32_t *labels)
{
    int64_t i = threadIdx.x;
    for (; i + 3 * THREADS < len; i += 4 * THREADS) {
        int32_t u[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; j++) u[j] = adj[s + i + j * THREADS];
#pragma unroll
        for (int j = 0; j < 4; j++) l[j] = labels[u[j]];
#pragma unroll
        for (int j = 0; j < 4; j++) lp_insert<__HIP_MEMORY_SCOPE_WORKGROUP>(tab, bits, l[j], 1);
    }
    for (; i < len; i += THREADS) lp_insert<__HIP_MEMORY_SCOPE_WORKGROUP>(tab, bits, labels[adj[s + i]], 1);
}

// ---- medium rows: one workgroup per row, LDS table ----
template <int THREADS, int SLOTS>
__global__ __launch_bounds__(THREADS) void vgl_k_lp_table(const int32_t *rows, const int32_t *n_rows, const int64_t *rowptr, const int32_t *adj, lp_io io)
{
    __shared__ unsigned long long tab[SLOTS];
    __shared__ unsigned long long s_red[THREADS / 64];
    constexpr int MAX_BITS = __builtin_ctz(SLOTS);
    const int32_t n = *n_rows;
    lp_acc acc;
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const int32_t v = rows[r];
        const int64_t s = rowptr[v], deg = rowptr[v + 1] - s;
        const int bits = lp_table_bits(deg, MAX_BITS);
        for (int i = threadIdx.x; i < (1 << bits); i += THREADS) tab[i] = 0;
        __syncthreads();
        lp_count_lds<THREADS>(tab, bits, adj, s, deg, io.labels);
        __syncthreads();
        uint64_t key = 0;
        for (int i = threadIdx.x; i < (1 << bits); i += THREADS) key = max(key, (uint64_t)tab[i]);
        key = lp_block_max<THREADS>(key, s_red);
        if (threadIdx.x == 0) acc.decide(io, v, key);
        __syncthreads();                                     // the table is cleared for the next row only after everyone has read it
    }
    acc.flush(io);
}

// ---- hubs ----
struct lp_hub_sched {
    const int32_t *row;         // per hub
    const int32_t *efirst;      // per hub: first edge chunk
    const int32_t *rfirst;      // per hub: first reduction chunk
    const int64_t *tbl;         // per hub: first slot of its table, relative to its batch
    const int32_t *tbits;       // per hub: log2 of its table's slots
    const int32_t *echunk_hub;  // per edge chunk
    const int32_t *rchunk_hub;  // per reduction chunk
};

// one workgroup per chunk of a hub's edges: LDS table of the chunk, then every distinct label with its count into the hub's global table
__global__ __launch_bounds__(LP_WIDE) void vgl_k_lp_hub_count(int32_t chunk0, lp_hub_sched hs, int32_t chunk_edges, const uint64_t *active,
                                                                 const int64_t *rowptr, const int32_t *adj, const int32_t *labels, unsigned long long *tables)
{
    __shared__ unsigned long long tab[LP_T1K_SLOTS];
    const int32_t k = chunk0 + blockIdx.x, h = hs.echunk_hub[k], v = hs.row[h];
    if (active && !lp_bit(active, v)) return;
    const int64_t rs = rowptr[v], re = rowptr[v + 1];
    const int64_t s = rs + (int64_t)(k - hs.efirst[h]) * chunk_edges, len = min((int64_t)chunk_edges, re - s);
    const int bits = lp_table_bits(len, 13);
    for (int i = threadIdx.x; i < (1 << bits); i += LP_WIDE) tab[i] = 0;
    __syncthreads();
    lp_count_lds<LP_WIDE>(tab, bits, adj, s, len, labels);
    __syncthreads();
    unsigned long long *g = tables + hs.tbl[h];
    const int gbits = hs.tbits[h];
    for (int i = threadIdx.x; i < (1 << bits); i += LP_WIDE) {
        const unsigned long long e = tab[i];
        if (e) lp_insert<__HIP_MEMORY_SCOPE_AGENT>(g, gbits, lp_key_label(e), (uint32_t)(e >> 32));
    }
}

// one workgroup per LP_RCHUNK slots of a hub's table: max into best[hub], and the slots are left at 0 for the next batch / iteration
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_hub_reduce(int32_t chunk0, lp_hub_sched hs, const uint64_t *active, unsigned long long *tables,
                                                                  unsigned long long *best)
{
    __shared__ unsigned long long s_red[VGL_WAVES];
    const int32_t k = chunk0 + blockIdx.x, h = hs.rchunk_hub[k];
    if (active && !lp_bit(active, hs.row[h])) return;
    const int64_t slots = (int64_t)1 << hs.tbits[h], off = (int64_t)(k - hs.rfirst[h]) * LP_RCHUNK;
    const int n = (int)min((int64_t)LP_RCHUNK, slots - off);
    unsigned long long *t = tables + hs.tbl[h] + off;
    uint64_t key = 0;
    for (int i = threadIdx.x; i < n; i += VGL_BLOCK) {
        key = max(key, (uint64_t)t[i]);
        t[i] = 0;
    }
    key = lp_block_max<VGL_BLOCK>(key, s_red);
    if (threadIdx.x == 0 && key) atomicMax(best + h, (unsigned long long)key);
}

__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_hub_decide(int32_t nhubs, const int32_t *hub_row, const uint64_t *active, unsigned long long *best, lp_io io)
{
    lp_acc acc;
    for (int32_t h = blockIdx.x * VGL_BLOCK + threadIdx.x; h - (int32_t)threadIdx.x < nhubs; h += gridDim.x * VGL_BLOCK) {
        if (h >= nhubs) continue;
        const int32_t v = hub_row[h];
        if (active && !lp_bit(active, v)) continue;
        const uint64_t key = best[h];
        best[h] = 0;
        acc.decide(io, v, key);
    }
    acc.flush(io);
}

// ---- classes ----
// ids (nullptr: 0 .. n-1) -> per-class lists at out + off[c]; cnt[c] counts.  off == nullptr: count only.  act (optional): rows / edges counted.
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_classify(const int32_t *ids, const int32_t *n_ptr, int32_t n_fixed, const int64_t *rowptr, lp_bounds b,
                                                                const int32_t *off, int32_t *cnt, int32_t *out, int64_t *act)
{
    __shared__ int32_t s32[VGL_WAVES];
    __shared__ int32_t s_base[LP_NCLS];
    const int32_t n = n_ptr ? *n_ptr : n_fixed;
    int64_t rows = 0, edges = 0;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < n; base += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t i = base + threadIdx.x;
        int32_t v = -1;
        int cls = -1;
        if (i < n) {
            v = ids ? ids[i] : (int32_t)i;
            const int64_t d = rowptr[v + 1] - rowptr[v];
            cls = lp_class_of(d, b);
            if (cls >= 0) { rows++; edges += d; }
        }
        int rank = 0;
        for (int c = 0; c < LP_NCLS; c++) {
            int total = 0;
            const int r = vgl_block_excl_add(cls == c ? 1 : 0, s32, &total);
            if (cls == c) rank = r;
            if (threadIdx.x == 0) s_base[c] = total ? atomicAdd(cnt + c, total) : 0;
        }
        __syncthreads();
        if (off && cls >= 0 && cls != LP_HUB) out[off[cls] + s_base[cls] + rank] = v;
        __syncthreads();
    }
    if (act) {
        rows = vgl_wave_reduce_add(rows);
        edges = vgl_wave_reduce_add(edges);
        if (vgl_lane() == 0 && rows) {
            atomicAdd(reinterpret_cast<unsigned long long *>(act + LP_ACT_ROWS), (unsigned long long)rows);
            atomicAdd(reinterpret_cast<unsigned long long *>(act + LP_ACT_EDGES), (unsigned long long)edges);
        }
    }
}

// rows with more than `thr` entries (unordered) and, for a list of rows, their (start, end) offsets
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_big_rows(int32_t n, const int64_t *rowptr, int64_t thr, int32_t *cnt, int32_t *out)
{
    for (int32_t v = blockIdx.x * VGL_BLOCK + threadIdx.x; v < n; v += gridDim.x * VGL_BLOCK)
        if (rowptr[v + 1] - rowptr[v] > thr) out[atomicAdd(cnt, 1)] = v;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_row_ranges(int32_t n, const int32_t *rows, const int64_t *rowptr, int64_t *se)
{
    for (int32_t i = blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += gridDim.x * VGL_BLOCK) {
        se[2 * (int64_t)i] = rowptr[rows[i]];
        se[2 * (int64_t)i + 1] = rowptr[rows[i] + 1];
    }
}

// ---- iteration plumbing ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_init(int32_t V, const int32_t *init, int32_t *labels)
{
    for (int32_t v = blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += gridDim.x * VGL_BLOCK) labels[v] = init ? init[v] : v;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_apply(int32_t V, const uint64_t *changed, const int32_t *next, int32_t *labels)
{
    for (int32_t v = blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += gridDim.x * VGL_BLOCK)
        if (lp_bit(changed, v)) labels[v] = next[v];
}
__device__ __forceinline__ void lp_mark(uint64_t *active, int32_t u)
{
    const unsigned long long bit = 1ull << (u & 63);
    if (!(active[u >> 6] & bit)) atomicOr(reinterpret_cast<unsigned long long *>(active) + (u >> 6), bit);
}
// changed vertices with at most `big` reverse entries: 16 lanes per vertex
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_push(const int32_t *chg, const int64_t *rowptr, const int32_t *adj, int64_t big, uint64_t *active)
{
    const int32_t n = chg[0];
    const int gi = threadIdx.x & 15;
    for (int64_t i = ((int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x) / 16; i < n; i += (int64_t)gridDim.x * VGL_BLOCK / 16) {
        const int32_t v = chg[1 + i];
        const int64_t s = rowptr[v], e = rowptr[v + 1];
        if (e - s > big) continue;
        for (int64_t p = s + gi; p < e; p += 16) lp_mark(active, adj[p]);
    }
}
// the larger rows: a static schedule of LP_PUSH_CHUNK-edge chunks over every row with more than `big` entries; chunks of unchanged rows return
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_lp_push_big(const int32_t *chunk_row, const int64_t *chunk_start, const int64_t *rowptr, const int32_t *adj,
                                                                const uint64_t *changed, uint64_t *active)
{
    const int32_t v = chunk_row[blockIdx.x];
    if (!lp_bit(changed, v)) return;
    const int64_t s = chunk_start[blockIdx.x], e = min(rowptr[v + 1], s + LP_PUSH_CHUNK);
    for (int64_t p = s + threadIdx.x; p < e; p += VGL_BLOCK) lp_mark(active, adj[p]);
}

template <class T> int lp_h2d(vgl_hip_ctx *c, T *d, const std::vector<T> &h)
{
    if (!h.empty()) VGL_HIP_TRY(hipMemcpyAsync(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, c->stream));
    return 0;
}

}  // namespace

// Degree classes of one stored CSR (cached on the graph, freed with it): the rows of each class, the hub schedule, and the schedule of the
// push over this CSR's large rows (used when this CSR is the reverse of the one whose labels are counted).
struct vgl_lp_cache {
    int64_t key[6] = {-1, -1, -1, -1, -1, -1};   // the switches it was built under
    lp_bounds b{};
    int32_t V = 0;
    vgl_dev<int32_t> rows;                       // V: the rows of class c at [off[c], off[c] + size[c])
    vgl_dev<int32_t> d_off, d_size;              // LP_NCLS each (device)
    int32_t off[LP_NCLS + 1] = {}, size[LP_NCLS] = {};
    int64_t nz_rows = 0;                         // rows with at least one entry
    // hubs
    int32_t nhubs = 0, n_echunks = 0, n_rchunks = 0, hub_chunk = 0;
    vgl_dev<int32_t> hub_i32;                    // row | efirst | rfirst | tbits (nhubs each) | echunk_hub | rchunk_hub
    vgl_dev<int64_t> hub_tbl;
    struct batch { int32_t e0, e1, r0, r1; };
    std::vector<batch> batches;
    int64_t table_slots = 0;                     // slots of the largest batch
    // push over this CSR
    int64_t push_big = 0;
    int32_t n_pchunks = 0;
    vgl_dev<int32_t> pchunk_row;
    vgl_dev<int64_t> pchunk_start;
    lp_hub_sched sched() const
    {
        const int32_t *p = hub_i32;
        return lp_hub_sched{p, p + nhubs, p + 2 * nhubs, hub_tbl, p + 3 * nhubs, p + 4 * nhubs, p + 4 * nhubs + n_echunks};
    }
};

template <> void vgl_cache_free(vgl_lp_cache *p) { delete p; }

namespace {

void lp_switches(vgl_hip_ctx *c, int64_t key[6])
{
    key[0] = vgl_env_int(c, "VGL_LP_LIGHT", 32, 0, 64);
    key[1] = vgl_env_int(c, "VGL_LP_WAVE", 512, key[0], 512);
    key[2] = vgl_env_int(c, "VGL_LP_MEDIUM", 4096, key[1], 4096);
    key[3] = vgl_env_int(c, "VGL_LP_HUB_CHUNK", 4096, 64, 4096);
    key[4] = vgl_env_int(c, "VGL_LP_HUB_SCRATCH_KB", 256 * 1024, 1, (int64_t)1 << 30) * 1024;
    key[5] = vgl_env_int(c, "VGL_LP_PUSH_BIG", 256, 16, (int64_t)1 << 40);
}

// rows of the CSR with more than thr entries, ascending, with their (start, end)
int lp_big_rows(vgl_hip_ctx *c, const vgl_dir_csr &d, int32_t V, int64_t thr, int32_t *d_tmp, std::vector<int32_t> &rows, std::vector<int64_t> &se)
{
    VGL_HIP_TRY(hipMemsetAsync(d_tmp, 0, sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(vgl_k_lp_big_rows, dim3((unsigned)std::min<int64_t>(LP_MAX_GRID, vgl_ceil_div(V, VGL_BLOCK))), dim3(VGL_BLOCK), 0, c->stream,
                       V, d.rowptr, thr, d_tmp, d_tmp + 1);
    VGL_HIP_TRY(hipGetLastError());
    int32_t n = 0;
    VGL_HIP_TRY(hipMemcpyAsync(&n, d_tmp, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    rows.resize((size_t)n);
    se.resize(2 * (size_t)n);
    if (n == 0) return 0;
    VGL_HIP_TRY(hipMemcpyAsync(rows.data(), d_tmp + 1, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    std::sort(rows.begin(), rows.end());
    VGL_TRY(lp_h2d(c, d_tmp + 1, rows));
    int64_t *d_se = reinterpret_cast<int64_t *>(d_tmp) + ((size_t)n + 2) / 2;       // (8-byte aligned, after the list at d_tmp + 1)
    hipLaunchKernelGGL(vgl_k_lp_row_ranges, dim3((unsigned)std::min<int64_t>(LP_MAX_GRID, vgl_ceil_div(n, VGL_BLOCK))), dim3(VGL_BLOCK), 0, c->stream,
                       n, (const int32_t *)(d_tmp + 1), d.rowptr, d_se);
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipMemcpyAsync(se.data(), d_se, sizeof(int64_t) * se.size(), hipMemcpyDeviceToHost, c->stream));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int lp_build(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_dir_csr &d, const int64_t key[6], vgl_cache<vgl_lp_cache> &out)
{
    const int32_t V = g->V;
    std::unique_ptr<vgl_lp_cache> p(new vgl_lp_cache());
    std::copy(key, key + 6, p->key);
    p->b = lp_bounds{(int)key[0], (int)key[1], (int)key[2]};
    p->V = V;
    p->hub_chunk = (int32_t)key[3];
    p->push_big = key[5];
    VGL_TRY(p->rows.alloc((size_t)V));
    VGL_TRY(p->d_off.alloc(LP_NCLS));
    VGL_TRY(p->d_size.alloc(LP_NCLS));
    // classes: count, offsets, scatter (ids in ascending order within each workgroup's range)
    const unsigned grid = (unsigned)std::min<int64_t>(LP_MAX_GRID, vgl_ceil_div(V, VGL_BLOCK));
    VGL_HIP_TRY(hipMemsetAsync(p->d_size, 0, sizeof(int32_t) * LP_NCLS, c->stream));
    hipLaunchKernelGGL(vgl_k_lp_classify, dim3(grid), dim3(VGL_BLOCK), 0, c->stream, (const int32_t *)nullptr, (const int32_t *)nullptr, V, d.rowptr, p->b,
                       (const int32_t *)nullptr, p->d_size, (int32_t *)nullptr, (int64_t *)nullptr);
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipMemcpyAsync(p->size, p->d_size, sizeof(p->size), hipMemcpyDeviceToHost, c->stream));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    p->off[0] = 0;
    for (int k = 0; k < LP_NCLS; k++) { p->off[k + 1] = p->off[k] + p->size[k]; p->nz_rows += p->size[k]; }
    VGL_HIP_TRY(hipMemcpyAsync(p->d_off, p->off, sizeof(int32_t) * LP_NCLS, hipMemcpyHostToDevice, c->stream));
    VGL_HIP_TRY(hipMemsetAsync(p->d_size, 0, sizeof(int32_t) * LP_NCLS, c->stream));
    hipLaunchKernelGGL(vgl_k_lp_classify, dim3(grid), dim3(VGL_BLOCK), 0, c->stream, (const int32_t *)nullptr, (const int32_t *)nullptr, V, d.rowptr, p->b,
                       (const int32_t *)p->d_off, p->d_size, p->rows, (int64_t *)nullptr);
    VGL_HIP_TRY(hipGetLastError());
    // hubs: sorted ids from the host, edge chunks, table sizes, batches within the scratch cap (a hub larger than the cap is a batch of its own)
    vgl_dev<int32_t> d_tmp;
    VGL_TRY(d_tmp.alloc((size_t)V * 6 + 16));
    std::vector<int32_t> rows;
    std::vector<int64_t> se;
    VGL_TRY(lp_big_rows(c, d, V, p->b.medium, d_tmp, rows, se));
    const int32_t nh = (int32_t)rows.size();
    std::vector<int32_t> efirst, rfirst, tbits, echunk_hub, rchunk_hub;
    std::vector<int64_t> tbl;
    int64_t batch_slots = 0;
    const int64_t cap_slots = key[4] / 8;
    for (int32_t h = 0; h < nh; h++) {
        const int64_t deg = se[2 * (size_t)h + 1] - se[2 * (size_t)h];
        const int bits = lp_table_bits(deg, 32);
        const int64_t slots = (int64_t)1 << bits;
        if (p->batches.empty() || (batch_slots > 0 && batch_slots + slots > cap_slots)) {
            p->batches.push_back({(int32_t)echunk_hub.size(), 0, (int32_t)rchunk_hub.size(), 0});
            batch_slots = 0;
        }
        efirst.push_back((int32_t)echunk_hub.size());
        rfirst.push_back((int32_t)rchunk_hub.size());
        tbits.push_back(bits);
        tbl.push_back(batch_slots);
        for (int64_t k = 0; k < vgl_ceil_div(deg, p->hub_chunk); k++) echunk_hub.push_back(h);
        for (int64_t k = 0; k < vgl_ceil_div(slots, LP_RCHUNK); k++) rchunk_hub.push_back(h);
        batch_slots += slots;
        p->batches.back().e1 = (int32_t)echunk_hub.size();
        p->batches.back().r1 = (int32_t)rchunk_hub.size();
        p->table_slots = std::max(p->table_slots, batch_slots);
    }
    p->nhubs = nh;
    p->n_echunks = (int32_t)echunk_hub.size();
    p->n_rchunks = (int32_t)rchunk_hub.size();
    std::vector<int32_t> packed(rows);
    for (auto *v : {&efirst, &rfirst, &tbits, &echunk_hub, &rchunk_hub}) packed.insert(packed.end(), v->begin(), v->end());
    VGL_TRY(p->hub_i32.alloc(packed.size()));
    VGL_TRY(p->hub_tbl.alloc(tbl.size()));
    VGL_TRY(lp_h2d(c, p->hub_i32.p, packed));
    VGL_TRY(lp_h2d(c, p->hub_tbl.p, tbl));
    // push schedule over this CSR: chunks of the rows with more than push_big entries
    VGL_TRY(lp_big_rows(c, d, V, p->push_big, d_tmp, rows, se));
    std::vector<int32_t> prow;
    std::vector<int64_t> pstart;
    for (size_t i = 0; i < rows.size(); i++)
        for (int64_t s = se[2 * i]; s < se[2 * i + 1]; s += LP_PUSH_CHUNK) { prow.push_back(rows[i]); pstart.push_back(s); }
    p->n_pchunks = (int32_t)prow.size();
    VGL_TRY(p->pchunk_row.alloc(prow.size()));
    VGL_TRY(p->pchunk_start.alloc(pstart.size()));
    VGL_TRY(lp_h2d(c, p->pchunk_row.p, prow));
    VGL_TRY(lp_h2d(c, p->pchunk_start.p, pstart));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    out.reset(p.release());
    return 0;
}

// the cache of stored direction `dir` (0 out, 1 in) under the current switches
int lp_ensure(vgl_hip_ctx *c, vgl_hip_graph *g, int dir, vgl_lp_cache **out)
{
    const vgl_dir_csr &d = dir ? g->in : g->out;
    int64_t key[6];
    lp_switches(c, key);
    auto &slot = g->lp[dir];
    if (slot && std::equal(key, key + 6, slot->key)) { *out = slot.get(); return 0; }
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    slot.reset();
    VGL_TRY(lp_build(c, g, d, key, slot));
    *out = slot.get();
    return 0;
}

unsigned lp_grid(int64_t work, int64_t per_block) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(LP_MAX_GRID, vgl_ceil_div(work, per_block))); }

// one compute pass over the rows listed per class (rows / counts on the device; sizes = host upper bounds)
int lp_compute(vgl_hip_ctx *c, const vgl_dir_csr &d, const vgl_lp_cache &k, const int32_t *rows, const int32_t *d_counts, const uint64_t *active,
               unsigned long long *tables, unsigned long long *best, const lp_io &io)
{
    const int32_t *sz = k.size;
    const int64_t *rp = d.rowptr;
    const int32_t *adj = d.adj;
#define LP_LIGHT(cls, G)                                                                                                                        \
    if (sz[cls]) {                                                                                                                              \
        vgl_timed_launch tl(c, "lp_light");                                                                                                     \
        hipLaunchKernelGGL(vgl_k_lp_light<G>, dim3(lp_grid(sz[cls], VGL_BLOCK / G)), dim3(VGL_BLOCK), 0, c->stream, rows + k.off[cls], d_counts + cls, rp, adj, io); \
    }
    LP_LIGHT(0, 4) LP_LIGHT(1, 8) LP_LIGHT(2, 16) LP_LIGHT(3, 32) LP_LIGHT(4, 64)
#undef LP_LIGHT
    if (sz[5]) {
        vgl_timed_launch tl(c, "lp_table64");
        hipLaunchKernelGGL((vgl_k_lp_table<64, LP_T64_SLOTS>), dim3(lp_grid(sz[5], 1)), dim3(64), 0, c->stream, rows + k.off[5], d_counts + 5, rp, adj, io);
    }
    if (sz[6]) {
        vgl_timed_launch tl(c, "lp_table1k");
        hipLaunchKernelGGL((vgl_k_lp_table<LP_WIDE, LP_T1K_SLOTS>), dim3(lp_grid(sz[6], 1)), dim3(LP_WIDE), 0, c->stream, rows + k.off[6], d_counts + 6, rp, adj, io);
    }
    if (k.nhubs) {
        vgl_timed_launch tl(c, "lp_hubs");
        const lp_hub_sched hs = k.sched();
        for (const auto &b : k.batches) {
            hipLaunchKernelGGL(vgl_k_lp_hub_count, dim3((unsigned)(b.e1 - b.e0)), dim3(LP_WIDE), 0, c->stream, b.e0, hs, k.hub_chunk, active, rp, adj, io.labels, tables);
            hipLaunchKernelGGL(vgl_k_lp_hub_reduce, dim3((unsigned)(b.r1 - b.r0)), dim3(VGL_BLOCK), 0, c->stream, b.r0, hs, active, tables, best);
        }
        hipLaunchKernelGGL(vgl_k_lp_hub_decide, dim3(lp_grid(k.nhubs, VGL_BLOCK)), dim3(VGL_BLOCK), 0, c->stream, k.nhubs, hs.row, active, best, io);
    }
    VGL_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int vgl_hip_lp_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int direction)
{
    if (!c || !g) VGL_FAIL("lp_prepare: null argument");
    if (direction != 0 && direction != 1) VGL_FAIL("lp_prepare: direction must be 0 (out) or 1 (in)");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("lp_prepare: graph handle must own all rows (LP has no sharded form)");
    if (direction == 1 && !g->in.rowptr) VGL_FAIL("lp_prepare: direction IN needs the incoming CSR");
    vgl_lp_cache *k = nullptr;
    VGL_TRY(lp_ensure(c, g, direction, &k));
    if ((direction ? g->out : g->in).rowptr) VGL_TRY(lp_ensure(c, g, 1 - direction, &k));     // the reverse: its push schedule
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_lp_run(vgl_hip_ctx *c, vgl_hip_graph *g, int direction, int mode, int symmetric, int max_iterations, const int32_t *d_init,
                   int32_t *d_labels, int64_t *changed_history, vgl_hip_lp_stats *stats)
{
    if (!c || !g || !d_labels) VGL_FAIL("lp_run: null argument");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("lp_run: graph handle must own all rows (LP has no sharded form)");
    if (direction != 0 && direction != 1) VGL_FAIL("lp_run: direction must be 0 (out) or 1 (in)");
    if (mode != VGL_LP_ALL_ACTIVE && mode != VGL_LP_FRONTIER && mode != VGL_LP_AUTO) VGL_FAIL("lp_run: unknown mode");
    if (max_iterations < 0) VGL_FAIL("lp_run: max_iterations must not be negative");
    if (direction == 1 && !g->in.rowptr) VGL_FAIL("lp_run: direction IN needs the incoming CSR");
    const int rdir = symmetric ? direction : 1 - direction;               // the CSR whose rows list who reads a vertex's label
    const bool have_rev = (rdir ? g->in : g->out).rowptr != nullptr;
    if (mode == VGL_LP_FRONTIER && !have_rev) VGL_FAIL("lp_run: FRONTIER needs the reverse CSR (the incoming one for OUT) or symmetric != 0");
    const bool frontier = mode != VGL_LP_ALL_ACTIVE && have_rev;
    const vgl_dir_csr &d = direction ? g->in : g->out;
    const vgl_dir_csr &rv = rdir ? g->in : g->out;
    const int32_t V = g->V;
    const int64_t words = vgl_ceil_div(V, 64) + 1;
    vgl_hip_lp_stats st;
    memset(&st, 0, sizeof(st));

    hipLaunchKernelGGL(vgl_k_lp_init, dim3(lp_grid(V, VGL_BLOCK)), dim3(VGL_BLOCK), 0, c->stream, V, d_init, d_labels);
    VGL_HIP_TRY(hipGetLastError());
    if (max_iterations == 0) {
        VGL_HIP_TRY(hipStreamSynchronize(c->stream));
        if (stats) *stats = st;
        return 0;
    }
    vgl_lp_cache *k = nullptr, *kr = nullptr;
    VGL_TRY(lp_ensure(c, g, direction, &k));
    if (frontier) VGL_TRY(lp_ensure(c, g, rdir, &kr));
    if (rdir == direction) kr = k;

    // scratch, once per call
    vgl_dev<int32_t> next, chg, act, flist, fcnt;
    vgl_dev<uint64_t> changed, active;
    vgl_dev<int64_t> cnt;
    vgl_dev<unsigned long long> tables, best;
    VGL_TRY(next.alloc(c->stream, (size_t)V));
    VGL_TRY(changed.alloc(c->stream, (size_t)words));
    VGL_TRY(cnt.alloc(c->stream, LP_NCNT));
    VGL_TRY(tables.alloc(c->stream, (size_t)k->table_slots));
    VGL_TRY(best.alloc(c->stream, (size_t)k->nhubs));
    if (frontier) {
        VGL_TRY(chg.alloc(c->stream, (size_t)V + 1));
        VGL_TRY(act.alloc(c->stream, (size_t)V + 1));
        VGL_TRY(flist.alloc(c->stream, (size_t)V));
        VGL_TRY(fcnt.alloc(c->stream, LP_NCLS));
        VGL_TRY(active.alloc(c->stream, (size_t)words));
    }
    VGL_HIP_TRY(hipMemsetAsync(changed, 0, sizeof(uint64_t) * (size_t)words, c->stream));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int64_t) * LP_NCNT, c->stream));
    if (k->table_slots) VGL_HIP_TRY(hipMemsetAsync(tables, 0, sizeof(uint64_t) * (size_t)k->table_slots, c->stream));
    if (k->nhubs) VGL_HIP_TRY(hipMemsetAsync(best, 0, sizeof(uint64_t) * (size_t)k->nhubs, c->stream));
    const lp_io io{d_labels, next, changed, have_rev ? rv.rowptr : nullptr, cnt};
    const double share = [&] { const char *s = vgl_env(c, "VGL_LP_FRONTIER_SHARE"); return (s && *s) ? atof(s) : 0.05; }();

    bool use_front = false;                                          // the first iteration evaluates every row
    int64_t h[LP_NCNT] = {0, 0, 0, 0};
    for (int it = 0; it < max_iterations; it++) {
        if (use_front) VGL_TRY(lp_compute(c, d, *k, flist, fcnt, active, tables, best, io));
        else VGL_TRY(lp_compute(c, d, *k, k->rows, k->d_size, nullptr, tables, best, io));
        VGL_HIP_TRY(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        VGL_HIP_TRY(hipStreamSynchronize(c->stream));                // the one synchronisation of an iteration
        st.iterations++;
        st.changed_last = h[LP_CHANGED];
        if (changed_history) changed_history[it] = h[LP_CHANGED];
        if (use_front) {
            st.frontier_steps++;
            st.rows_processed += h[LP_ACT_ROWS];
            st.edges_examined += h[LP_ACT_EDGES];
            st.algorithmic_bytes += 16 * h[LP_ACT_ROWS] + 8 * h[LP_ACT_EDGES] + 8 * (int64_t)words;
        } else {
            st.rows_processed += k->nz_rows;
            st.edges_examined += d.edges;
            st.algorithmic_bytes += 16 * (int64_t)V + 8 * d.edges;     // row offsets, labels read + written; adjacency + gathered labels
        }
        if (h[LP_CHANGED] == 0) { st.converged = 1; break; }
        const bool last = it + 1 == max_iterations;
        use_front = !last && frontier && (double)h[LP_PUSHED] <= share * (double)d.edges;
        if (use_front) {                                             // the rows that read a changed label: push over the reverse CSR
            VGL_TRY(vgl_zero_words(c, active, words));
            VGL_TRY(vgl_bitmap_to_ids(c, words, changed, 0, V, chg));
            {
                vgl_timed_launch tl(c, "lp_push");
                hipLaunchKernelGGL(vgl_k_lp_push, dim3(lp_grid(h[LP_CHANGED], VGL_BLOCK / 16)), dim3(VGL_BLOCK), 0, c->stream, (const int32_t *)chg,
                                   rv.rowptr, rv.adj, kr->push_big, active);
                if (kr->n_pchunks)
                    hipLaunchKernelGGL(vgl_k_lp_push_big, dim3((unsigned)kr->n_pchunks), dim3(VGL_BLOCK), 0, c->stream, (const int32_t *)kr->pchunk_row,
                                       (const int64_t *)kr->pchunk_start, rv.rowptr, rv.adj, (const uint64_t *)changed, active);
                VGL_HIP_TRY(hipGetLastError());
            }
            VGL_TRY(vgl_bitmap_to_ids(c, words, active, 0, V, act));
            VGL_HIP_TRY(hipMemsetAsync(fcnt, 0, sizeof(int32_t) * LP_NCLS, c->stream));
            VGL_HIP_TRY(hipMemsetAsync(cnt + LP_ACT_ROWS, 0, 2 * sizeof(int64_t), c->stream));
            vgl_timed_launch tl(c, "lp_frontier");
            hipLaunchKernelGGL(vgl_k_lp_classify, dim3(lp_grid(V, VGL_BLOCK)), dim3(VGL_BLOCK), 0, c->stream, (const int32_t *)(act + 1), (const int32_t *)act,
                               0, d.rowptr, k->b, (const int32_t *)k->d_off, fcnt, flist, cnt);
            VGL_HIP_TRY(hipGetLastError());
            st.algorithmic_bytes += 8 * h[LP_CHANGED] + 4 * h[LP_PUSHED] + 8 * (int64_t)words;
        }
        {
            vgl_timed_launch tl(c, "lp_apply");
            hipLaunchKernelGGL(vgl_k_lp_apply, dim3(lp_grid(V, VGL_BLOCK)), dim3(VGL_BLOCK), 0, c->stream, V, (const uint64_t *)changed, (const int32_t *)next, d_labels);
            VGL_HIP_TRY(hipGetLastError());
        }
        st.algorithmic_bytes += 8 * (int64_t)words + 8 * h[LP_CHANGED];
        VGL_TRY(vgl_zero_words(c, changed, words));
        VGL_HIP_TRY(hipMemsetAsync(cnt, 0, 2 * sizeof(int64_t), c->stream));
    }
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    if (stats) *stats = st;
    return 0;
}

}  // extern "C"
