// tri.hip -- triangle counting (global count, per-vertex counts, undirected degrees) on the simple undirected graph underlying the stored outgoing
// CSR.  The contract is written out in include/vgl_hip.h.  (`tc` in this tree is transitive closure; triangle counting is `tri` everywhere.)
//
// Prepare (once per graph, cached on the handle): the oriented CSR of the simple graph, from the key sort of simple.hip (vgl_simple_build_oriented):
// every edge once, in the row of its lower endpoint under the total order  (stored out-degree [+ in-degree when the incoming CSR exists], id),  every
// row ascending BY VERTEX ID and free of duplicates.  The intersections compare vertex ids, so no rank array is kept: the order only decides which
// endpoint owns an edge.  Degree order bounds every oriented row by about sqrt(2 E').
//
// Count: triangles = sum over oriented edges (a, b) of |N+(a) & N+(b)|; {a < b < c in the order} is found once, at (a, b) with witness c.
// Rows a are split by oriented out-degree d = d+(a) (heaviest first inside a class):
//   light (d <= VGL_TRI_LIGHT, <= 64)  : a wave takes 64 rows, expands their edges through an LDS owner map, and a group of G = 4 / 8 / 16 / 32 lanes
//                                        (by d) takes one edge (a, b): the lanes stride over the shorter of N+(a), N+(b) and binary-search the longer.
//   table (d <= VGL_TRI_TABLE, <= 8192): one 256-thread workgroup per row: N+(a) into an LDS open-addressing set (pow2 >= 2 d slots; 2048 slots up to
//                                        VGL_TRI_TABLE_SMALL, <= 1024, else 16384), then groups of 16 lanes stream N+(b) for every b of N+(a) and probe.
//   huge  (d > VGL_TRI_TABLE)          : the same kernel over (row, chunk) units: VGL_TRI_HUGE_CHUNK (<= 8192) entries of N+(a) per LDS set, the N+(b)
//                                        streams repeated per chunk.  No scratch block; a row of any length is ceil(d / chunk) workgroups.
// Hits are summed in registers, per wave, then one 64-bit atomic per wave.  With per-vertex counts (template parameter) the witness takes one atomic
// per hit, b one per edge, a one per edge (light) or per unit (table, huge); without them none of these atomics exist in the kernel.
#include "vgl_simple.h"
#include "vgl_prim.h"
#include <cstring>
#include <algorithm>
#include <cstdlib>
#include <vector>

namespace {

constexpr int TRI_NCLS = 7;                 // light G = 4, 8, 16, 32 | table 2048 | table 16384 | huge
constexpr int TRI_TS = 4, TRI_TL = 5, TRI_HUGE = 6;
constexpr int TRI_LIGHT_MAX = 64;           // owner map: 64 rows x 64 entries of one byte per wave
constexpr int TRI_SLOTS_S = 2048, TRI_SLOTS_L = 16384;
constexpr int TRI_TG = 16;                  // lanes that stream one N+(b) in the table kernels
constexpr int64_t TRI_MAX_GRID = 1 << 20;
enum { TRI_C_TRI = 0, TRI_C_WORK = 1, TRI_NCNT = 2 };

struct tri_bounds { int light, small, table; };

__host__ __device__ inline int tri_class_of(int64_t d, tri_bounds b)
{
    if (d <= 0) return -1;
    if (d <= b.light) return d <= 8 ? 0 : d <= 16 ? 1 : d <= 32 ? 2 : 3;
    if (d <= b.small) return TRI_TS;
    if (d <= b.table) return TRI_TL;
    return TRI_HUGE;
}

// every lane of the wave, once, at the end of a count kernel
__device__ __forceinline__ void tri_flush(int64_t *cnt, int64_t tri, int64_t work)
{
    tri = vgl_wave_reduce_add(tri);
    work = vgl_wave_reduce_add(work);
    if (vgl_lane() == 0) {
        if (tri) vgl_atomic_add64(cnt + TRI_C_TRI, tri);
        if (work) vgl_atomic_add64(cnt + TRI_C_WORK, work);
    }
}

// ---- prepare ----
// sort key of a row: class << 28 | (2^28 - 1 - min(d, 2^28 - 1)): classes ascending, heaviest rows first inside a class; rows without entries last
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_tri_classify(int32_t V, const int64_t *rowptr, tri_bounds b, uint32_t *keys, int32_t *ids, int32_t *sizes)
{
    __shared__ int s_n[TRI_NCLS];
    if (threadIdx.x < TRI_NCLS) s_n[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int64_t d = rowptr[v + 1] - rowptr[v];
        const int cls = tri_class_of(d, b);
        keys[v] = cls < 0 ? 0xFFFFFFFFu : (uint32_t)cls << 28 | (0x0FFFFFFFu - (uint32_t)min(d, (int64_t)0x0FFFFFFF));
        ids[v] = (int32_t)v;
        if (cls >= 0) atomicAdd(&s_n[cls], 1);
    }
    __syncthreads();
    if (threadIdx.x < TRI_NCLS && s_n[threadIdx.x]) atomicAdd(sizes + threadIdx.x, s_n[threadIdx.x]);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_tri_row_degrees(int32_t n, const int32_t *rows, const int64_t *rowptr, int32_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) out[i] = (int32_t)(rowptr[rows[i] + 1] - rowptr[rows[i]]);
}

// ---- count: light rows ----
template <int G, bool PV>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_tri_light(const int32_t *rows, int32_t n, const int64_t *rowptr, const int32_t *adj, int64_t *cnt, int64_t *pv)
{
    constexpr int EPW = 64 / G;                                 // edges per wave and round
    __shared__ uint8_t s_owner[VGL_WAVES][64 * TRI_LIGHT_MAX];  // edge slot of the wave's 64 rows -> the lane that holds its row
    uint8_t *owner = s_owner[vgl_wave()];
    const int lane = vgl_lane(), gi = lane & (G - 1);
    int64_t tri = 0, work = 0;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < n; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t r = base + threadIdx.x;
        int32_t a = 0;
        int64_t sa = 0;
        int da = 0;
        if (r < n) {
            a = rows[r];
            sa = rowptr[a];
            da = min((int)(rowptr[a + 1] - sa), TRI_LIGHT_MAX);      // (the class bound; the clamp keeps the map in bounds whatever the list holds)
        }
        const int incl = vgl_wave_incl_add(da), excl = incl - da;
        const int total = __shfl(incl, 63);
        __syncthreads();                                             // the map of the round before has been read
        for (int k = 0; k < da; k++) owner[excl + k] = (uint8_t)lane;
        __syncthreads();
        for (int t0 = 0; t0 < total; t0 += EPW) {                    // (uniform over the wave: the shuffles below read every lane)
            const int t = t0 + lane / G;
            const bool valid = t < total;
            const int own = valid ? owner[t] : 0;
            const int32_t ea = __shfl(a, own);
            const int64_t esa = __shfl(sa, own);
            const int eda = __shfl(da, own), eex = __shfl(excl, own);
            int hits = 0;
            int32_t b = 0;
            if (valid) {
                b = adj[esa + (t - eex)];
                const int64_t sb = rowptr[b];
                const int db = (int)min(rowptr[b + 1] - sb, (int64_t)0x7FFFFFFF);
                const bool a_short = eda <= db;
                const int64_t ss = a_short ? esa : sb, ls = a_short ? sb : esa;
                const int sn = a_short ? eda : db, ln = a_short ? db : eda;
                if (gi == 0) work += sn;
                for (int i = gi; i < sn; i += G) {
                    const int32_t x = adj[ss + i];
                    if (vgl_contains(adj, ls, ln, x)) {
                        hits++;
                        if (PV) vgl_atomic_add64(pv + x, 1);
                    }
                }
            }
            tri += hits;
            if (PV) {
#pragma unroll
                for (int o = G / 2; o > 0; o >>= 1) hits += __shfl_xor(hits, o);
                if (valid && gi == 0 && hits) { vgl_atomic_add64(pv + ea, hits); vgl_atomic_add64(pv + b, hits); }
            }
        }
    }
    tri_flush(cnt, tri, work);
}

// ---- count: table and huge rows ----
// unit u: row unit_row[u]; entries [chunk * chunk_len, + chunk_len) of N+(a) go into the LDS set (unit_chunk == nullptr: the whole row, chunk 0), and
// every N+(b), b in the WHOLE of N+(a), is streamed against it.  chunk_len <= SLOTS / 2.
template <int SLOTS, bool PV>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_tri_table(const int32_t *unit_row, const int32_t *unit_chunk, int32_t n_units, int chunk_len, const int64_t *rowptr,
                                                              const int32_t *adj, int64_t *cnt, int64_t *pv)
{
    __shared__ int32_t s_tab[SLOTS];
    __shared__ int64_t s_red[VGL_WAVES];
    const int gi = threadIdx.x & (TRI_TG - 1);
    int64_t tri = 0, work = 0;
    for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {      // (uniform over the workgroup)
        const int32_t a = unit_row[u];
        const int64_t sa = rowptr[a];
        const int64_t da = rowptr[a + 1] - sa;
        const int64_t c0 = unit_chunk ? (int64_t)unit_chunk[u] * chunk_len : 0;
        const int cn = (int)max((int64_t)0, min(da - c0, (int64_t)min(chunk_len, SLOTS / 2)));
        int bits = 6;
        while ((1 << bits) < 2 * cn) bits++;                         // <= log2(SLOTS) because cn <= SLOTS / 2
        const uint32_t mask = (1u << bits) - 1u;
        __syncthreads();                                             // the set of the unit before has been probed
        for (int i = threadIdx.x; i <= (int)mask; i += VGL_BLOCK) s_tab[i] = -1;
        __syncthreads();
        for (int i = threadIdx.x; i < cn; i += VGL_BLOCK) {
            const int32_t x = adj[sa + c0 + i];
            uint32_t h = vgl_hash(x, bits);
            while (atomicCAS(&s_tab[h], -1, x) != -1) h = (h + 1) & mask;      // (no duplicates in a row: a taken slot holds another id)
        }
        __syncthreads();
        int64_t unit_hits = 0;
        for (int64_t j = threadIdx.x / TRI_TG; j < da; j += VGL_BLOCK / TRI_TG) {
            const int32_t b = adj[sa + j];
            const int64_t sb = rowptr[b], db = rowptr[b + 1] - sb;
            int hits = 0;
            for (int64_t p = gi; p < db; p += TRI_TG) {
                const int32_t x = adj[sb + p];
                uint32_t h = vgl_hash(x, bits);
                for (int32_t y = s_tab[h]; y != -1; y = s_tab[h]) {
                    if (y == x) {
                        hits++;
                        if (PV) vgl_atomic_add64(pv + x, 1);
                        break;
                    }
                    h = (h + 1) & mask;
                }
            }
            if (gi == 0) work += db;
            unit_hits += hits;
            if (PV) {                                                 // (the group's 16 lanes share j: they are all here)
#pragma unroll
                for (int o = TRI_TG / 2; o > 0; o >>= 1) hits += __shfl_xor(hits, o);
                if (gi == 0 && hits) vgl_atomic_add64(pv + b, hits);
            }
        }
        tri += unit_hits;
        if (PV) {
            const int64_t row_hits = vgl_block_reduce_add(unit_hits, s_red);
            if (threadIdx.x == 0 && row_hits) vgl_atomic_add64(pv + a, row_hits);
        }
    }
    tri_flush(cnt, tri, work);
}

}  // namespace

// The oriented CSR of a graph and the class lists of its rows (cached on the handle, freed with it)
struct vgl_tri_cache {
    int32_t V = 0;
    vgl_simple_csr csr;                          // nnz = E'; max_deg: the longest oriented row
    // classes (rebuilt when the switches change; the oriented CSR stays)
    int64_t key[4] = {-1, -1, -1, -1};
    tri_bounds b{};
    vgl_dev<int32_t> rows;                       // V: the rows of class c at [off[c], off[c] + size[c])
    int32_t off[TRI_NCLS + 1] = {}, size[TRI_NCLS] = {};
    int32_t n_units = 0, chunk_len = 0;          // huge: (row, chunk) units
    vgl_dev<int32_t> unit_row, unit_chunk;
};

template <> void vgl_cache_free(vgl_tri_cache *p) { delete p; }

namespace {

// the class lists under the switches `key`
int tri_build_classes(vgl_hip_ctx *c, vgl_tri_cache *p, const int64_t key[4])
{
    hipStream_t st = c->stream;
    const int32_t V = p->V;
    p->rows.reset(); p->unit_row.reset(); p->unit_chunk.reset();
    p->n_units = 0;
    std::fill(p->key, p->key + 4, -1);
    p->b = tri_bounds{(int)key[0], (int)key[1], (int)key[2]};
    p->chunk_len = (int32_t)key[3];
    std::fill(p->size, p->size + TRI_NCLS, 0);
    std::fill(p->off, p->off + TRI_NCLS + 1, 0);
    VGL_TRY(p->rows.alloc((size_t)V));
    if (V > 0) {
        vgl_dev<uint32_t> k_in, k_out;
        vgl_dev<int32_t> ids, sizes;
        VGL_TRY(k_in.alloc(st, (size_t)V));
        VGL_TRY(k_out.alloc(st, (size_t)V));
        VGL_TRY(ids.alloc(st, (size_t)V));
        VGL_TRY(sizes.alloc(st, TRI_NCLS));
        VGL_HIP_TRY(hipMemsetAsync(sizes, 0, sizeof(int32_t) * TRI_NCLS, st));
        hipLaunchKernelGGL(vgl_k_tri_classify, dim3(vgl_grid(V, VGL_BLOCK, 16384)), dim3(VGL_BLOCK), 0, st, V, (const int64_t *)p->csr.rowptr.p, p->b, k_in, ids, sizes);
        VGL_HIP_TRY(hipGetLastError());
        vgl_scratch temp;
        VGL_TRY(vgl_sort_pairs(c, temp, k_in.p, k_out.p, ids.p, p->rows.p, (size_t)V, 0, 32));
        VGL_HIP_TRY(hipMemcpyAsync(p->size, sizes, sizeof(p->size), hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        for (int k = 0; k < TRI_NCLS; k++) p->off[k + 1] = p->off[k] + p->size[k];
        const int32_t nh = p->size[TRI_HUGE];
        if (nh) {                                                     // (row, chunk) units of the huge rows, heaviest row first
            vgl_dev<int32_t> d_deg;
            VGL_TRY(d_deg.alloc(st, (size_t)nh));
            const int32_t *hrows = p->rows + p->off[TRI_HUGE];
            hipLaunchKernelGGL(vgl_k_tri_row_degrees, dim3(vgl_grid(nh, VGL_BLOCK, 16384)), dim3(VGL_BLOCK), 0, st, nh, hrows, (const int64_t *)p->csr.rowptr.p, d_deg);
            VGL_HIP_TRY(hipGetLastError());
            std::vector<int32_t> hr((size_t)nh), hd((size_t)nh), ur, uc;
            VGL_HIP_TRY(hipMemcpyAsync(hr.data(), hrows, sizeof(int32_t) * (size_t)nh, hipMemcpyDeviceToHost, st));
            VGL_HIP_TRY(hipMemcpyAsync(hd.data(), d_deg, sizeof(int32_t) * (size_t)nh, hipMemcpyDeviceToHost, st));
            VGL_HIP_TRY(hipStreamSynchronize(st));
            for (int32_t i = 0; i < nh; i++)
                for (int64_t k = 0; k < vgl_ceil_div(hd[(size_t)i], p->chunk_len); k++) { ur.push_back(hr[(size_t)i]); uc.push_back((int32_t)k); }
            p->n_units = (int32_t)ur.size();
            VGL_TRY(p->unit_row.alloc(ur.size()));
            VGL_TRY(p->unit_chunk.alloc(uc.size()));
            VGL_HIP_TRY(hipMemcpyAsync(p->unit_row, ur.data(), sizeof(int32_t) * ur.size(), hipMemcpyHostToDevice, st));
            VGL_HIP_TRY(hipMemcpyAsync(p->unit_chunk, uc.data(), sizeof(int32_t) * uc.size(), hipMemcpyHostToDevice, st));
            VGL_HIP_TRY(hipStreamSynchronize(st));
        }
    }
    std::copy(key, key + 4, p->key);
    return 0;
}

int tri_ensure(vgl_hip_ctx *c, vgl_hip_graph *g, vgl_tri_cache **out, bool *built)
{
    int64_t key[4];
    key[0] = vgl_env_int(c, "VGL_TRI_LIGHT", 64, 0, TRI_LIGHT_MAX);
    key[1] = vgl_env_int(c, "VGL_TRI_TABLE_SMALL", 1024, key[0], TRI_SLOTS_S / 2);
    key[2] = vgl_env_int(c, "VGL_TRI_TABLE", 8192, key[1], TRI_SLOTS_L / 2);
    key[3] = vgl_env_int(c, "VGL_TRI_HUGE_CHUNK", 8192, 16, TRI_SLOTS_L / 2);
    *built = false;
    if (!g->tri) {
        vgl_cache<vgl_tri_cache> p(new vgl_tri_cache());
        p->V = g->V;
        VGL_TRY(vgl_simple_build_oriented(c, g, &p->csr));
        g->tri = std::move(p);
        *built = true;
    }
    if (!std::equal(key, key + 4, g->tri->key)) {
        VGL_HIP_TRY(hipStreamSynchronize(c->stream));
        VGL_TRY(tri_build_classes(c, g->tri.get(), key));
    }
    *out = g->tri.get();
    return 0;
}

template <bool PV>
int tri_count(vgl_hip_ctx *c, const vgl_tri_cache &k, int64_t *cnt, int64_t *pv)
{
    const int64_t *rp = k.csr.rowptr;
    const int32_t *adj = k.csr.adj;
#define TRI_LIGHT(cls, G)                                                                                                                          \
    if (k.size[cls]) {                                                                                                                             \
        vgl_timed_launch tl(c, "tri_light");                                                                                                       \
        hipLaunchKernelGGL((vgl_k_tri_light<G, PV>), dim3(vgl_grid(k.size[cls], VGL_BLOCK, TRI_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream, (const int32_t *)(k.rows + k.off[cls]), \
                           k.size[cls], rp, adj, cnt, pv);                                                                                          \
    }
    TRI_LIGHT(0, 4) TRI_LIGHT(1, 8) TRI_LIGHT(2, 16) TRI_LIGHT(3, 32)
#undef TRI_LIGHT
    if (k.size[TRI_TS]) {
        vgl_timed_launch tl(c, "tri_table");
        hipLaunchKernelGGL((vgl_k_tri_table<TRI_SLOTS_S, PV>), dim3(vgl_grid(k.size[TRI_TS], 1, TRI_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream,
                           (const int32_t *)(k.rows + k.off[TRI_TS]), (const int32_t *)nullptr, k.size[TRI_TS], TRI_SLOTS_S / 2, rp, adj, cnt, pv);
    }
    if (k.size[TRI_TL]) {
        vgl_timed_launch tl(c, "tri_table");
        hipLaunchKernelGGL((vgl_k_tri_table<TRI_SLOTS_L, PV>), dim3(vgl_grid(k.size[TRI_TL], 1, TRI_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream,
                           (const int32_t *)(k.rows + k.off[TRI_TL]), (const int32_t *)nullptr, k.size[TRI_TL], TRI_SLOTS_L / 2, rp, adj, cnt, pv);
    }
    if (k.n_units) {
        vgl_timed_launch tl(c, "tri_huge");
        hipLaunchKernelGGL((vgl_k_tri_table<TRI_SLOTS_L, PV>), dim3(vgl_grid(k.n_units, 1, TRI_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream, (const int32_t *)k.unit_row,
                           (const int32_t *)k.unit_chunk, k.n_units, k.chunk_len, rp, adj, cnt, pv);
    }
    VGL_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int vgl_hip_tri_prepare(vgl_hip_ctx *c, vgl_hip_graph *g)
{
    if (!c || !g) VGL_FAIL("tri_prepare: null argument");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("tri_prepare: graph handle must own all rows (triangle counting has no sharded form)");
    vgl_tri_cache *k = nullptr;
    bool built = false;
    VGL_TRY(tri_ensure(c, g, &k, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int vgl_hip_tri_run(vgl_hip_ctx *c, vgl_hip_graph *g, int64_t *triangles, int64_t *d_per_vertex, int32_t *d_degree, vgl_hip_tri_stats *stats)
{
    if (!c || !g) VGL_FAIL("tri_run: null argument");
    if (!triangles) VGL_FAIL("tri_run: triangles must not be NULL");
    if (g->row_begin != 0 || g->row_end != g->V) VGL_FAIL("tri_run: graph handle must own all rows (triangle counting has no sharded form)");
    vgl_tri_cache *k = nullptr;
    bool built = false;
    VGL_TRY(tri_ensure(c, g, &k, &built));
    const int32_t V = g->V;
    vgl_dev<int64_t> cnt;                                             // the one scratch draw: the two counters
    VGL_TRY(cnt.alloc(c->stream, TRI_NCNT));
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int64_t) * TRI_NCNT, c->stream));
    if (d_per_vertex && V > 0) VGL_HIP_TRY(hipMemsetAsync(d_per_vertex, 0, sizeof(int64_t) * (size_t)V, c->stream));
    if (d_degree && V > 0) VGL_HIP_TRY(hipMemcpyAsync(d_degree, k->csr.deg, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToDevice, c->stream));
    if (d_per_vertex) VGL_TRY(tri_count<true>(c, *k, cnt, d_per_vertex));
    else VGL_TRY(tri_count<false>(c, *k, cnt, nullptr));
    int64_t h[TRI_NCNT] = {0, 0};
    VGL_HIP_TRY(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    *triangles = h[TRI_C_TRI];
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->triangles = h[TRI_C_TRI];
        stats->undirected_edges = k->csr.nnz;
        stats->intersections = k->csr.nnz;
        stats->elements_examined = h[TRI_C_WORK];
        stats->algorithmic_bytes = 8 * (int64_t)V + 4 * k->csr.nnz + 4 * h[TRI_C_WORK];
        stats->max_oriented_degree = k->csr.max_deg;
        stats->prepared_now = built ? 1 : 0;
        stats->rows_light = (int64_t)k->size[0] + k->size[1] + k->size[2] + k->size[3];
        stats->rows_table = (int64_t)k->size[TRI_TS] + k->size[TRI_TL];
        stats->rows_huge = k->size[TRI_HUGE];
    }
    return 0;
}

}  // extern "C"
