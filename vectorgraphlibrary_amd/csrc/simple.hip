// simple.hip -- the simple undirected graph under the stored outgoing CSR: the one key-sort CSR builder (oriented for tri, symmetric for kcore, ktruss
// and msf) and the handle's cache of the symmetric CSR, its edge numbering and the edge of every stored entry.  vgl_simple.h; DESIGN section 18.
//
// Builder: every stored entry (u, v), u != v, yields 64-bit keys  row << 32 | entry  (which ones: the key functor).  The keys are sorted and
// deduplicated (vgl_prim.h), in pieces of consecutive rows when all of them would need more scratch than the cap; a row with more keys
// than the cap is a piece of its own.  The sorted keys ARE the CSR: row = high half, entry = low half, every row ascending and free of duplicates,
// the pieces appended in row order.
//
// Edge ids: up[u] = entries of row u of the symmetric CSR above u (one binary search per row), their exclusive scan = the id of the first edge whose
// lower endpoint is u, and eid[slot]: a slot (u, v), u < v, is edge up_off[u] + its rank among the upper entries of row u; a slot (v, u) finds the slot
// (u, v) by a binary search of row u.  eu / ev are written by the upper slots.  slot_eid: a stored entry (r, c) is found in row r by a binary search.
#include "vgl_simple.h"
#include "vgl_prim.h"
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

template <> void vgl_cache_free(vgl_simple_cache *p) { delete p; }

namespace {

constexpr int64_t SG_MAX_GRID = 16384;      // workgroups of a grid-stride kernel
constexpr int64_t SG_IDS_GRID = 8192;       // ... of the two kernels of the edge numbering

// ---- the keys of a stored entry (u, v), u != v, both in [0, V): how many, and which ----
// oriented: lower << 32 | higher under ord[v] = degree << 32 | v (u is below v iff ord[u] < ord[v])
struct sg_oriented_keys {
    static constexpr int MAX = 1;
    const uint64_t *ord;
    __device__ __forceinline__ int operator()(int32_t u, int32_t v, uint64_t *key) const
    {
        const bool u_low = ord[u] < ord[v];
        key[0] = (uint64_t)(uint32_t)(u_low ? u : v) << 32 | (uint32_t)(u_low ? v : u);
        return 1;
    }
};
struct sg_symmetric_keys {
    static constexpr int MAX = 2;
    __device__ __forceinline__ int operator()(int32_t u, int32_t v, uint64_t *key) const
    {
        key[0] = (uint64_t)(uint32_t)u << 32 | (uint32_t)v;
        key[1] = (uint64_t)(uint32_t)v << 32 | (uint32_t)u;
        return 2;
    }
};
// the keys of stored entry e; none for a loop
template <class KEYS>
__device__ __forceinline__ int sg_keys_of(const int64_t *rp, const int32_t *adj, int32_t V, int64_t e, const KEYS &keys_of, uint64_t *key)
{
    const int32_t u = vgl_row_of(rp, V, e), v = adj[e];
    if (u == v || v < 0 || v >= V) return 0;
    return keys_of(u, v, key);
}

// ---- the builder's kernels ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_order(int32_t V, const int64_t *out_rp, const int64_t *in_rp, uint64_t *ord)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        int64_t d = out_rp[v + 1] - out_rp[v];
        if (in_rp) d += in_rp[v + 1] - in_rp[v];
        ord[v] = (uint64_t)min(d, (int64_t)0xFFFFFFFFll) << 32 | (uint64_t)v;
    }
}
// keys per row before deduplication (only when the keys do not fit one piece)
template <class KEYS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_count(int32_t V, int64_t E, const int64_t *rp, const int32_t *adj, KEYS keys_of, int32_t *per_row)
{
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < E; e += (int64_t)gridDim.x * VGL_BLOCK) {
        uint64_t key[KEYS::MAX];
        const int n = sg_keys_of(rp, adj, V, e, keys_of, key);
        for (int j = 0; j < n; j++) atomicAdd(per_row + (key[j] >> 32), 1);
    }
}
// the keys whose row is in [v0, v1), appended in any order (the sort follows); never more than cap are written
template <class KEYS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_emit(int32_t V, int64_t E, const int64_t *rp, const int32_t *adj, KEYS keys_of, int32_t v0, int32_t v1, uint64_t *keys,
                                                                unsigned long long *n_keys, int64_t cap)
{
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < E; e += (int64_t)gridDim.x * VGL_BLOCK) {
        uint64_t key[KEYS::MAX];
        const int n = sg_keys_of(rp, adj, V, e, keys_of, key);
        for (int j = 0; j < n; j++) {
            const int32_t row = (int32_t)(key[j] >> 32);
            if (row < v0 || row >= v1) continue;
            const unsigned long long pos = atomicAdd(n_keys, 1ull);
            if ((int64_t)pos < cap) keys[pos] = key[j];
        }
    }
}
// sorted unique keys of a piece -> entries [base, base + n) of the adjacency; entry_deg (oriented CSR): the entry's vertex takes one add per entry
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_fill(const uint64_t *keys, int64_t n, int64_t base, int32_t *adj, int64_t adj_cap, int32_t V, int32_t *entry_deg)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t x = (int32_t)(uint32_t)keys[i];
        if (base + i < adj_cap) adj[base + i] = x;
        if (entry_deg && x >= 0 && x < V) atomicAdd(entry_deg + x, 1);
    }
}
// rowptr[r] = base + (keys of the piece below row r), r in [v0, v1]
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_rowptr(const uint64_t *keys, int64_t n, int32_t v0, int32_t v1, int64_t base, int64_t *rowptr)
{
    for (int64_t r = v0 + (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; r <= v1; r += (int64_t)gridDim.x * VGL_BLOCK) {
        const uint64_t first = (uint64_t)r << 32;
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < first) lo = mid + 1; else hi = mid;
        }
        rowptr[r] = base + lo;
    }
}
// deg[v] += length of row v (deg holds the fill kernel's adds, or zeros); the longest row
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_degrees(int32_t V, const int64_t *rowptr, int32_t *deg, int32_t *max_deg)
{
    int m = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int d = (int)(rowptr[v + 1] - rowptr[v]);
        deg[v] += d;
        m = max(m, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if (vgl_lane() == 0 && m) atomicMax(max_deg, m);
}

// ---- the kernels of the edge numbering ----
// up[u] = entries of row u above u (u < V); up[V] = 0
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_upper(int32_t V, const int64_t *rowptr, const int32_t *adj, int32_t *up)
{
    for (int64_t u = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; u <= V; u += (int64_t)gridDim.x * VGL_BLOCK) {
        int32_t n = 0;
        if (u < V) {
            int64_t lo = rowptr[u];
            const int64_t end = rowptr[u + 1];
            int64_t hi = end;
            while (lo < hi) {                                         // the first entry above u
                const int64_t mid = lo + (hi - lo) / 2;
                if (adj[mid] <= (int32_t)u) lo = mid + 1; else hi = mid;
            }
            n = (int32_t)(end - lo);
        }
        up[u] = n;
    }
}
// eid of every slot; eu / ev from the upper slots.  up_off: the exclusive scan of up (V + 1 entries; up_off[V] = E').
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_eid(int32_t V, int64_t nnz, const int64_t *rowptr, const int32_t *adj, const int32_t *up_off, int32_t *eid,
                                                               int32_t *eu, int32_t *ev, int32_t ne)
{
    for (int64_t s = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; s < nnz; s += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t r = vgl_row_of(rowptr, V, s), c = adj[s];
        if (c < 0 || c >= V || c == r) continue;                      // (the builder leaves none of these)
        const int32_t lo = min(r, c), hi = max(r, c);
        const int64_t first_up = rowptr[lo + 1] - (up_off[lo + 1] - up_off[lo]);      // slot of the first upper entry of row lo
        const int64_t slot = r < c ? s : vgl_slot_of(adj, first_up, rowptr[lo + 1], hi);
        if (slot < 0) continue;                                       // (a symmetric CSR has the slot)
        const int32_t id = up_off[lo] + (int32_t)(slot - first_up);
        if (id < 0 || id >= ne) continue;
        eid[s] = id;
        if (r < c) { eu[id] = lo; ev[id] = hi; }
    }
}
// slot_eid of every stored outgoing entry: the entry (r, c), c != r, is found in row r of the symmetric CSR; eid of that slot
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_simple_slot_eid(int32_t V, int64_t E, const int64_t *out_rp, const int32_t *out_adj, const int64_t *rowptr, const int32_t *adj,
                                                                    const int32_t *eid, int32_t ne, int32_t *slot_eid)
{
    for (int64_t s = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; s < E; s += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t r = vgl_row_of(out_rp, V, s), c = out_adj[s];
        int32_t id = -1;
        if (c >= 0 && c < V && c != r) {
            const int64_t slot = vgl_slot_of(adj, rowptr[r], rowptr[r + 1], c);
            if (slot >= 0) id = eid[slot];
            if (id >= ne) id = -1;                                    // (the numbering has no such id)
        }
        slot_eid[s] = id;
    }
}

// ---- the builder ----
// cap_mb: the key buffers (in + out, 8 bytes per key each) of one piece stay within it.  entry_deg: the fill kernel's hook.  slot: the timing slot of
// the degrees launch, or nullptr.  who prefixes the internal-error messages.
template <class KEYS>
int sg_build(vgl_hip_ctx *c, vgl_hip_graph *g, const KEYS &keys_of, int64_t cap_mb, bool entry_deg, const char *slot, const char *who, vgl_simple_csr *p)
{
    const int32_t V = g->V;
    const vgl_dir_csr &d = g->out;
    const int64_t E = d.edges, max_keys = KEYS::MAX * E;              // bounds the unique keys from above
    hipStream_t st = c->stream;
    VGL_TRY(p->rowptr.alloc((size_t)V + 1));
    VGL_TRY(p->deg.alloc((size_t)V));
    VGL_HIP_TRY(hipMemsetAsync(p->rowptr, 0, sizeof(int64_t) * ((size_t)V + 1), st));
    VGL_HIP_TRY(hipMemsetAsync(p->deg, 0, sizeof(int32_t) * (size_t)std::max(V, 1), st));
    p->nnz = 0;
    p->max_deg = 0;
    if (V <= 0 || E <= 0) {
        VGL_TRY(p->adj.alloc(1));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
    const int64_t cap_keys = std::max<int64_t>(1, cap_mb * (1 << 20) / 16);
    const unsigned grid_e = vgl_grid(E, VGL_BLOCK, SG_MAX_GRID);
    std::vector<int64_t> bounds{0, V};                                // pieces of consecutive rows (vgl_pieces.h)
    int64_t piece_keys = max_keys;
    if (max_keys > cap_keys) {
        vgl_dev<int32_t> per_row;
        VGL_TRY(per_row.alloc(st, (size_t)V));
        VGL_HIP_TRY(hipMemsetAsync(per_row, 0, sizeof(int32_t) * (size_t)V, st));
        hipLaunchKernelGGL(vgl_k_simple_count<KEYS>, dim3(grid_e), dim3(VGL_BLOCK), 0, st, V, E, d.rowptr, d.adj, keys_of, per_row.p);
        VGL_HIP_TRY(hipGetLastError());
        std::vector<int32_t> h((size_t)V);
        VGL_HIP_TRY(hipMemcpyAsync(h.data(), per_row, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        per_row.reset();
        piece_keys = std::max<int64_t>(vgl_plan_pieces(V, [&](int64_t v) { return (int64_t)h[(size_t)v]; }, cap_keys, &bounds), 1);
    }
    vgl_dev<uint64_t> keys_a, keys_b;
    vgl_dev<unsigned long long> n_keys;
    vgl_dev<size_t> n_unique;
    vgl_dev<int32_t> adj_tmp;                                         // max_keys entries: the right-sized adj is drawn once nnz is known
    VGL_TRY(keys_a.alloc(st, (size_t)piece_keys));
    VGL_TRY(keys_b.alloc(st, (size_t)piece_keys));
    VGL_TRY(n_keys.alloc(st, 1));
    VGL_TRY(n_unique.alloc(st, 1));
    VGL_TRY(adj_tmp.alloc(st, (size_t)max_keys));
    const int end_bit = 32 + vgl_index_bits(V);
    vgl_scratch temp;                                                 // sized for the largest piece here: the loop allocates nothing
    VGL_TRY(vgl_sort_keys(c, temp, keys_a.p, keys_b.p, (size_t)piece_keys, 0, end_bit, VGL_SIZE_ONLY));
    VGL_TRY(vgl_unique(c, temp, keys_b.p, keys_a.p, n_unique.p, (size_t)piece_keys, VGL_SIZE_ONLY));
    int64_t base = 0;
    for (size_t pc = 0; pc + 1 < bounds.size(); pc++) {
        const int32_t v0 = (int32_t)bounds[pc], v1 = (int32_t)bounds[pc + 1];
        VGL_HIP_TRY(hipMemsetAsync(n_keys, 0, sizeof(unsigned long long), st));
        hipLaunchKernelGGL(vgl_k_simple_emit<KEYS>, dim3(grid_e), dim3(VGL_BLOCK), 0, st, V, E, d.rowptr, d.adj, keys_of, v0, v1, keys_a.p, n_keys.p, piece_keys);
        VGL_HIP_TRY(hipGetLastError());
        unsigned long long nk = 0;
        VGL_HIP_TRY(hipMemcpyAsync(&nk, n_keys, sizeof(nk), hipMemcpyDeviceToHost, st));
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if ((int64_t)nk > piece_keys) VGL_FAIL((std::string(who) + ": a piece holds more keys than were counted for it").c_str());
        size_t nu = 0;
        if (nk) {
            VGL_TRY(vgl_sort_keys(c, temp, keys_a.p, keys_b.p, (size_t)nk, 0, end_bit));
            VGL_TRY(vgl_unique(c, temp, keys_b.p, keys_a.p, n_unique.p, (size_t)nk));
            VGL_HIP_TRY(hipMemcpyAsync(&nu, n_unique, sizeof(nu), hipMemcpyDeviceToHost, st));
            VGL_HIP_TRY(hipStreamSynchronize(st));
        }
        if (base + (int64_t)nu > max_keys) VGL_FAIL((std::string(who) + ": more entries than the stored ones can give").c_str());
        hipLaunchKernelGGL(vgl_k_simple_fill, dim3(vgl_grid((int64_t)nu, VGL_BLOCK, SG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, (const uint64_t *)keys_a.p, (int64_t)nu, base, adj_tmp.p,
                           max_keys, V, entry_deg ? p->deg.p : nullptr);
        hipLaunchKernelGGL(vgl_k_simple_rowptr, dim3(vgl_grid((int64_t)v1 - v0 + 1, VGL_BLOCK, SG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, (const uint64_t *)keys_a.p, (int64_t)nu, v0, v1,
                           base, p->rowptr.p);
        VGL_HIP_TRY(hipGetLastError());
        base += (int64_t)nu;
    }
    p->nnz = base;
    VGL_TRY(p->adj.alloc((size_t)base));
    if (base) VGL_HIP_TRY(hipMemcpyAsync(p->adj, adj_tmp, sizeof(int32_t) * (size_t)base, hipMemcpyDeviceToDevice, st));
    int32_t *d_max = reinterpret_cast<int32_t *>(n_keys.p);
    VGL_HIP_TRY(hipMemsetAsync(n_keys, 0, sizeof(unsigned long long), st));
    auto degrees = [&]() { hipLaunchKernelGGL(vgl_k_simple_degrees, dim3(vgl_grid(V, VGL_BLOCK, SG_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int64_t *)p->rowptr.p, p->deg.p, d_max); };
    if (slot) {
        vgl_timed_launch tl(c, slot);
        degrees();
    } else degrees();
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipMemcpyAsync(&p->max_deg, d_max, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// stage 2 of the cache: the numbering of the edges of k.csr
int sg_build_edge_ids(vgl_hip_ctx *c, int32_t V, vgl_simple_cache &k)
{
    const vgl_simple_csr &csr = k.csr;
    const int64_t ne = csr.nnz / 2;
    if (ne >= ((int64_t)1 << 31)) VGL_FAIL("ktruss_prepare: 2^31 or more undirected edges (edge ids are int32)");
    hipStream_t st = c->stream;
    k.ne = ne;
    VGL_TRY(k.eid.alloc((size_t)(2 * ne)));
    VGL_TRY(k.eu.alloc((size_t)ne));
    VGL_TRY(k.ev.alloc((size_t)ne));
    if (ne == 0) return 0;
    vgl_dev<int32_t> up, up_off;
    vgl_scratch temp;
    VGL_TRY(up.alloc(st, (size_t)V + 1));
    VGL_TRY(up_off.alloc(st, (size_t)V + 1));
    VGL_HIP_TRY(hipMemsetAsync(k.eid, 0, sizeof(int32_t) * (size_t)(2 * ne), st));
    {
        vgl_timed_launch tl(c, "ktruss_prepare");
        hipLaunchKernelGGL(vgl_k_simple_upper, dim3(vgl_grid((int64_t)V + 1, VGL_BLOCK, SG_IDS_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int64_t *)csr.rowptr.p, (const int32_t *)csr.adj.p, up.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_exclusive_scan(c, temp, up.p, up_off.p, (size_t)V + 1));
    {
        vgl_timed_launch tl(c, "ktruss_prepare");
        hipLaunchKernelGGL(vgl_k_simple_eid, dim3(vgl_grid(csr.nnz, VGL_BLOCK, SG_IDS_GRID)), dim3(VGL_BLOCK), 0, st, V, csr.nnz, (const int64_t *)csr.rowptr.p, (const int32_t *)csr.adj.p,
                           (const int32_t *)up_off.p, k.eid.p, k.eu.p, k.ev.p, (int32_t)ne);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// stage 3: the edge of every stored outgoing entry
int sg_build_slot_ids(vgl_hip_ctx *c, vgl_hip_graph *g, vgl_simple_cache &k)
{
    const int64_t E = g->out.edges;
    VGL_TRY(k.slot_eid.alloc((size_t)E));
    if (E == 0) return 0;
    {
        vgl_timed_launch tl(c, "msf_prepare");
        hipLaunchKernelGGL(vgl_k_simple_slot_eid, dim3(vgl_grid(E, VGL_BLOCK, SG_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream, g->V, E, g->out.rowptr, g->out.adj,
                           (const int64_t *)k.csr.rowptr.p, (const int32_t *)k.csr.adj.p, (const int32_t *)k.eid.p, (int32_t)k.ne, k.slot_eid.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

// the cache with its first `want` stages built; *built_now: stage `want` was missing
int sg_ensure(vgl_hip_ctx *c, vgl_hip_graph *g, int want, const vgl_simple_cache **out, bool *built_now)
{
    *built_now = !g->simple || g->simple->stages < want;
    if (!g->simple) {
        vgl_cache<vgl_simple_cache> k(new vgl_simple_cache());
        VGL_TRY(sg_build(c, g, sg_symmetric_keys{}, vgl_env_int(c, "VGL_KCORE_SORT_CAP_MB", 4096, 0, (int64_t)1 << 24), false, "kcore_csr", "kcore_prepare", &k->csr));
        k->stages = 1;
        g->simple = std::move(k);
    }
    vgl_simple_cache &k = *g->simple;
    if (k.stages < 2 && want >= 2) {
        VGL_TRY(sg_build_edge_ids(c, g->V, k));
        k.stages = 2;
    }
    if (k.stages < 3 && want >= 3) {
        VGL_TRY(sg_build_slot_ids(c, g, k));
        k.stages = 3;
    }
    *out = &k;
    return 0;
}

}  // namespace

int vgl_simple_build_oriented(vgl_hip_ctx *c, vgl_hip_graph *g, vgl_simple_csr *out)
{
    vgl_dev<uint64_t> ord;
    VGL_TRY(ord.alloc(c->stream, (size_t)g->V));
    if (g->V > 0) {
        hipLaunchKernelGGL(vgl_k_simple_order, dim3(vgl_grid(g->V, VGL_BLOCK, SG_MAX_GRID)), dim3(VGL_BLOCK), 0, c->stream, g->V, g->out.rowptr, g->in.rowptr, ord.p);
        VGL_HIP_TRY(hipGetLastError());
    }
    return sg_build(c, g, sg_oriented_keys{ord.p}, vgl_env_int(c, "VGL_TRI_SORT_CAP_MB", 4096, 0, (int64_t)1 << 24), true, nullptr, "tri_prepare", out);
}
int vgl_simple_ensure_csr(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_simple_cache **out, bool *built_now) { return sg_ensure(c, g, 1, out, built_now); }
int vgl_simple_ensure_edge_ids(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_simple_cache **out, bool *built_now) { return sg_ensure(c, g, 2, out, built_now); }
int vgl_simple_ensure_slot_ids(vgl_hip_ctx *c, vgl_hip_graph *g, const vgl_simple_cache **out, bool *built_now) { return sg_ensure(c, g, 3, out, built_now); }
