// bicc.hip -- biconnectivity of the simple undirected graph underlying the stored outgoing CSR: bridges, cut vertices (articulation points), the
// biconnected components (blocks) as a partition of the E' edges, and the 2-edge-connected components.  The contract is written out in
// include/vgl_hip.h; DESIGN section 20 has the rules, the kernel table and the bytes model.
//
// The symmetric simple CSR and the edge numbering (eid per slot, endpoints) are simple.hip's (vgl_simple_ensure_edge_ids), shared with kcore, ktruss
// and msf.  A run is the Tarjan-Vishkin reduction on a rooted BFS forest, in linear work and O(depth) launches:
//   roots     a lock-free union-find over the E' edges (the larger root is hooked under the smaller by compare-and-swap, so a find walks strictly
//             decreasing ids and the root of a class is its smallest vertex): the smallest vertex of every component is its root.
//   bfs       one level-synchronous top-down BFS seeded with all roots at once, one kernel per row class (short: 8 lanes per row, wave: a wavefront,
//             wg: a workgroup).  A vertex is claimed by a compare-and-swap on its level; the claimer writes the parent and appends the vertex to the
//             list of its class (vgl_wave_append).  The three lists are cumulative, so each holds its class in level order; the host reads the list
//             tails once per level and keeps the level offsets, which is all the later passes need: they make no host reads.
//   size      deepest level first: size[parent] += size[v].
//   pre       top level first: a root takes the running offset of its tree, a child  pre[p] + 1 + (what its earlier siblings took of cursor[p]).
//             The sibling order is arbitrary: all that is used is subtree(v) = [pre[v], pre[v] + size[v]).
//   local     per row, by class, one writer: low / high[v] = min / max of pre[v] and of pre[w] over the row's NON-TREE entries w.
//   lowhigh   deepest level first: integer atomicMin / atomicMax onto the parent, skipped when the slot already holds as good a value.
//   reset     one launch: the block and the 2-edge union-find as singletons, no edge counted, no smallest edge known (what the call asks for).
//   edge      one thread per edge.  Tree edge (child c, parent p): bridge iff low[c] >= pre[c] and high[c] < pre[c] + size[c]; a tree edge that is no
//             bridge unites c and p in the 2-edge union-find; if p is no root and subtree(c) has an exit past subtree(p), c and p are united in the
//             block union-find, whose elements are the tree edges named by their child.  A non-tree edge (a, b) unites a and b there: in a BFS forest
//             it never joins a vertex to its ancestor, so both ends name tree edges of the edge's block.
//   block     the block union-find is flattened; every edge offers its id to its class root (atomicMin, skipped when the slot is already smaller)
//             and is counted there (lanes of a wave that share a root go as one); a second pass writes the smallest id as the label.
//   art       per row, by class, one writer: a cut vertex is a row whose entries' edges carry two different labels.
//   twoecc    the 2-edge union-find flattened: the root is the smallest vertex of the class, which is the label.
// INVARIANT: inside one launch a word that another workgroup of that launch writes is read with an agent-scope atomic load or not at all; everything
// else crosses a kernel boundary.  No cooperative launch, no grid barrier, no wait on a flag: a union-find retry is a new find, never a spin.
#include "vgl_simple.h"
#include "vgl_rowclass.h"
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace {

typedef unsigned long long bi_cnt;
constexpr int64_t BI_MAX_GRID = 2048;            // workgroups of a grid-stride kernel
enum {
    BI_TAIL = 0,        // + class: vertices appended to the class list so far (cumulative)
    BI_ROWS = 3,        // + class: vertices per class
    BI_ROOTS = 6,       // connected components
    BI_BRIDGES = 7,
    BI_ARTS = 8,        // cut vertices
    BI_BLOCKS = 9,
    BI_LARGEST = 10,    // edges of the largest block
    BI_TWOECC = 11,     // 2-edge-connected components
    BI_TREES = 12,      // the running preorder offset of the trees
    BI_NCNT = 13
};
static_assert(BI_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

// the three class lists (cumulative over the levels); cap[c] = vertices of the class
struct bi_lists { int32_t *rows[VGL_RC_N]; int32_t cap[VGL_RC_N]; };
// one level (or all levels) of the lists: n[c] vertices from rows[c]
struct bi_slice { const int32_t *rows[VGL_RC_N]; int32_t n[VGL_RC_N]; };
__device__ __forceinline__ int32_t bi_slice_at(const bi_slice &s, int64_t i)
{
    return i < s.n[0] ? s.rows[0][i] : i < (int64_t)s.n[0] + s.n[1] ? s.rows[1][i - s.n[0]] : s.rows[2][i - s.n[0] - s.n[1]];
}
// every lane of the wave calls: the lanes with `want` append v to the list of its class
__device__ __forceinline__ void bi_append(bool want, int32_t v, int cls, const bi_lists &L, bi_cnt *tail)
{
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) {
        int32_t *const one[1] = {L.rows[c]};
        vgl_wave_append<1>(want && cls == c, v, 0, one, L.cap[c], tail + c);
    }
}

// ---- the union-find: parent[x] <= x always, a root is its own parent, the root of a class is its smallest id ----
// A find reads through agent-scope loads and splits the path behind it.  Only a non-root is ever stored to, and only with one of its ancestors, so a
// compare-and-swap on a root (the one place where two classes join) cannot be undone.
__device__ __forceinline__ int32_t bi_find(int32_t *parent, int32_t x)
{
    int32_t p = vgl_load_agent(parent + x);
    while (p != x) {
        const int32_t gp = vgl_load_agent(parent + p);
        if (gp != p) vgl_store_agent(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}
__device__ __forceinline__ void bi_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = bi_find(parent, a);
        b = bi_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }            // the larger root goes under the smaller
        if (atomicCAS(parent + a, a, b) == a) return;                 // lost: a has a parent now, the next find starts from it
    }
}

// Every lane of the wave calls (uniform control flow).  The lanes with `on` add val to arr[key]; returns what the slot held before the lane's own
// share.  The lanes that share the key of the first pending lane go as one atomic, twice over; what is left goes lane by lane.  (A hub with 10^5
// children is one key for whole waves.)
__device__ __forceinline__ int32_t bi_fetch_add_by_key(bool on, int32_t key, int32_t val, int32_t *arr)
{
    const int lane = vgl_lane();
    int32_t got = 0;
    for (int it = 0; it < 2; it++) {
        const unsigned long long rest = __ballot(on);
        if (!rest) break;                                             // (uniform)
        const int leader = __ffsll((long long)rest) - 1;
        const int32_t k0 = __shfl(key, leader);
        const bool same = on && key == k0;
        const int32_t x = same ? val : 0;
        const int32_t incl = vgl_wave_incl_add(x);
        const int32_t total = __shfl(incl, 63);
        int32_t base = 0;
        if (lane == leader) base = atomicAdd(arr + k0, total);
        base = __shfl(base, leader);
        if (same) { got = base + incl - x; on = false; }
    }
    if (on) got = atomicAdd(arr + key, val);
    return got;
}

// ---- init, roots, seed ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_init(int32_t V, const int32_t *deg, vgl_rc_bounds b, int32_t *uf, int32_t *level, int32_t *size, int32_t *cursor, bi_cnt *cnt)
{
    int64_t n[VGL_RC_N] = {0, 0, 0};
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        uf[v] = (int32_t)v;
        level[v] = -1;
        size[v] = 1;
        cursor[v] = 0;
        n[vgl_rc_class_of(deg[v], b)]++;
    }
#pragma unroll
    for (int c = 0; c < VGL_RC_N; c++) vgl_wave_flush_add(cnt + BI_ROWS + c, n[c]);
}
// what the passes per edge start from: the two union-finds as singletons, no edge counted, no smallest edge known (each may be NULL)
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_reset(int32_t V, int32_t *uf_two, int32_t *uf_block, int32_t *edges_of, uint32_t *min_edge)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        if (uf_two) uf_two[v] = (int32_t)v;
        if (uf_block) { uf_block[v] = (int32_t)v; edges_of[v] = 0; min_edge[v] = ~0u; }
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_unite_edges(int32_t ne, const int32_t *eu, const int32_t *ev, int32_t *uf)
{
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < ne; e += (int64_t)gridDim.x * VGL_BLOCK) bi_unite(uf, eu[e], ev[e]);
}
// out[v] = the root of v; roots: how many vertices are their own root (may be NULL).  out is an array of its own: the finds of other threads split
// paths as they go, and such a store into uf[v] may land after this thread's and put an ancestor that is no root in the place of the root.
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_flatten(int32_t V, int32_t *uf, int32_t *out, bi_cnt *roots)
{
    int64_t n = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t r = bi_find(uf, (int32_t)v);
        out[v] = r;
        n += r == (int32_t)v;
    }
    if (roots) vgl_wave_flush_add(roots, n);
}
// the roots (a vertex that is its own parent after the unite launch) are level 0
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_seed(int32_t V, const int32_t *uf, const int32_t *deg, vgl_rc_bounds b, int32_t *level, int32_t *parent, bi_lists L, bi_cnt *cnt)
{
    int64_t n = 0;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < V; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t v = base + threadIdx.x;
        const bool root = v < V && uf[v] == (int32_t)v;
        int cls = 0;
        if (root) {
            level[v] = 0;
            parent[v] = -1;
            cls = vgl_rc_class_of(deg[v], b);
            n++;
        }
        bi_append(root, (int32_t)v, cls, L, cnt + BI_TAIL);
    }
    vgl_wave_flush_add(cnt + BI_ROOTS, n);
}

// ---- the BFS levels ----
struct bi_bfs {
    const int64_t *rowptr;       // the symmetric CSR
    const int32_t *adj;
    const int32_t *deg;
    int32_t *level, *parent;
    bi_lists L;
    bi_cnt *cnt;
    vgl_rc_bounds b;
    int32_t next_level;
};
// one entry (v -> w): true for the lane that claimed w.  level[w] is -1 or the level of its claim, which is final.
__device__ __forceinline__ bool bi_visit(const bi_bfs &t, int32_t v, int32_t w)
{
    if (vgl_load_agent(t.level + w) >= 0) return false;
    if (atomicCAS(t.level + w, -1, t.next_level) != -1) return false;
    t.parent[w] = v;
    return true;
}
__device__ __forceinline__ void bi_bfs_entry(const bi_bfs &t, int32_t v, int64_t e, int64_t hi)      // every lane of the wave
{
    int32_t w = 0;
    bool app = false;
    int cls = 0;
    if (e < hi) {
        w = t.adj[e];
        app = bi_visit(t, v, w);
        if (app) cls = vgl_rc_class_of(t.deg[w], t.b);
    }
    bi_append(app, w, cls, t.L, t.cnt + BI_TAIL);
}
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_bfs(const int32_t *rows, int32_t n, bi_bfs t)
{
    using T = vgl_rc_team<CLS>;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        int32_t v = 0;
        int64_t lo = 0, hi = 0;
        if (i < n) {
            v = rows[i];
            lo = t.rowptr[v]; hi = t.rowptr[v + 1];
        }
        for (int64_t e = lo + T::lane(); __any(e < hi); e += T::LANES) bi_bfs_entry(t, v, e, hi);      // (uniform over the wave)
    }
}

// ---- subtree intervals: one launch per level over that level's slice ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_size(bi_slice s, const int32_t *parent, int32_t *size)
{
    const int64_t total = (int64_t)s.n[0] + s.n[1] + s.n[2];
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < total; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        const bool on = i < total;
        int32_t p = 0, sv = 0;
        if (on) {
            const int32_t v = bi_slice_at(s, i);
            p = parent[v];
            sv = size[v];
        }
        bi_fetch_add_by_key(on, p, sv, size);
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_pre(bi_slice s, int32_t roots, const int32_t *parent, const int32_t *size, int32_t *cursor, int32_t *pre, bi_cnt *trees)
{
    const int64_t total = (int64_t)s.n[0] + s.n[1] + s.n[2];
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < total; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        const bool on = i < total;
        int32_t v = 0, p = 0, sv = 0;
        if (on) {
            v = bi_slice_at(s, i);
            p = parent[v];
            sv = size[v];
        }
        if (roots) {                                                  // (uniform) a wave's trees take one stretch of the running offset
            const int32_t incl = vgl_wave_incl_add(sv);
            bi_cnt first = 0;
            if (vgl_lane() == 63 && incl) first = atomicAdd(trees, (bi_cnt)incl);
            first = __shfl(first, 63);
            if (on) pre[v] = (int32_t)first + incl - sv;
        } else {
            const int32_t before = bi_fetch_add_by_key(on, p, sv, cursor);
            if (on) pre[v] = pre[p] + 1 + before;
        }
    }
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_lowhigh(bi_slice s, const int32_t *parent, int32_t *low, int32_t *high)
{
    const int64_t total = (int64_t)s.n[0] + s.n[1] + s.n[2];
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t v = bi_slice_at(s, i), p = parent[v];
        const int32_t lv = low[v], hv = high[v];
        if (vgl_load_agent(low + p) > lv) atomicMin(low + p, lv);
        if (vgl_load_agent(high + p) < hv) atomicMax(high + p, hv);
    }
}

// ---- rows by class, the smallest and the largest of a value over the row's entries, one writer per row ----
// OP: ctx(v) -> what entry() needs of the row; entry(v, ctx, slot, mn, mx) folds one entry; finish(v, mn, mx) writes and returns what is counted;
// counter() -> where the counts go, or NULL.
template <int CLS, class OP>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_rows(const int32_t *rows, int32_t n, OP op)
{
    using T = vgl_rc_team<CLS>;
    int64_t acc = 0;
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const int64_t i = T::item(at);
        const bool has = i < n;
        int32_t v = 0, cx = 0, mn = INT_MAX, mx = INT_MIN;
        int64_t lo = 0, hi = 0;
        if (has) {
            v = rows[i];
            cx = op.ctx(v);
            lo = op.rowptr[v]; hi = op.rowptr[v + 1];
        }
        for (int64_t e = lo + T::lane(); e < hi; e += T::LANES) op.entry(v, cx, e, mn, mx);
        mn = T::min_of(mn);
        mx = T::max_of(mx);
        if (T::lead() && has) acc += op.finish(v, mn, mx);
    }
    if (op.counter()) vgl_wave_flush_add(op.counter(), acc);
}
// low / high before the levels fold them: pre[v] and pre[w] over the non-tree entries w of the row
struct bi_local_op {
    const int64_t *rowptr;
    const int32_t *adj, *parent, *pre;
    int32_t *low, *high;
    __device__ __forceinline__ int32_t ctx(int32_t v) const { return parent[v]; }
    __device__ __forceinline__ void entry(int32_t v, int32_t pv, int64_t e, int32_t &mn, int32_t &mx) const
    {
        const int32_t w = adj[e];
        if (pv == w || parent[w] == v) return;                        // a tree entry
        const int32_t x = pre[w];
        mn = min(mn, x); mx = max(mx, x);
    }
    __device__ __forceinline__ int finish(int32_t v, int32_t mn, int32_t mx) const
    {
        const int32_t x = pre[v];
        low[v] = min(mn, x);
        high[v] = max(mx, x);
        return 0;
    }
    __device__ __forceinline__ bi_cnt *counter() const { return nullptr; }
};
// a cut vertex: a row whose entries' edges carry two different labels
struct bi_art_op {
    const int64_t *rowptr;
    const int32_t *eid, *label;
    uint8_t *art;                // may be NULL: counted only
    bi_cnt *cnt;
    __device__ __forceinline__ int32_t ctx(int32_t) const { return 0; }
    __device__ __forceinline__ void entry(int32_t, int32_t, int64_t e, int32_t &mn, int32_t &mx) const
    {
        const int32_t x = label[eid[e]];
        mn = min(mn, x); mx = max(mx, x);
    }
    __device__ __forceinline__ int finish(int32_t v, int32_t mn, int32_t mx) const
    {
        const int a = mn < mx ? 1 : 0;                                // (an empty row: INT_MAX, INT_MIN)
        if (art) art[v] = (uint8_t)a;
        return a;
    }
    __device__ __forceinline__ bi_cnt *counter() const { return cnt + BI_ARTS; }
};

// ---- per edge ----
struct bi_edge {
    const int32_t *eu, *ev, *parent, *pre, *size, *low, *high;
    uint8_t *bridge;             // may be NULL
    int32_t *name;               // block pass: the vertex that names the edge's tree edge; NULL when the pass is skipped
    int32_t *uf_block;           // with name
    int32_t *uf_two;             // may be NULL
    bi_cnt *cnt;
};
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_edge(int32_t ne, bi_edge t)
{
    int64_t bridges = 0;
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < ne; e += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t a = t.eu[e], b = t.ev[e];
        int32_t c = -1, p = -1;
        if (t.parent[a] == b) { c = a; p = b; }
        else if (t.parent[b] == a) { c = b; p = a; }
        bool br = false;
        if (c >= 0) {
            const int32_t lc = t.low[c], hc = t.high[c], pc = t.pre[c];
            br = lc >= pc && hc < pc + t.size[c];
            bridges += br;
            if (!br && t.uf_two) bi_unite(t.uf_two, c, p);
            if (t.name) {
                t.name[e] = c;
                if (t.parent[p] >= 0) {                               // p is no root
                    const int32_t pp = t.pre[p];
                    if (lc < pp || hc >= pp + t.size[p]) bi_unite(t.uf_block, c, p);
                }
            }
        } else if (t.name) {
            t.name[e] = a;
            bi_unite(t.uf_block, a, b);
        }
        if (t.bridge) t.bridge[e] = br ? 1 : 0;
    }
    vgl_wave_flush_add(t.cnt + BI_BRIDGES, bridges);
}

// ---- blocks ----
// label[e]: the naming vertex on entry, the class root on exit; the root learns the smallest edge id and the number of edges of its class.  A thread
// keeps the count of its current root in a register and hands it over when the root changes (and at the end), and offers an edge id only at the start
// of such a stretch: the edges of a giant block reach its two words as a few atomics per wave, not as one load per edge and one add per 64 edges.
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_block_min(int32_t ne, int32_t *label, const int32_t *root, uint32_t *min_edge, int32_t *edges)
{
    int32_t cur = 0, n = 0;
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < ne; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t e = base + threadIdx.x;
        const bool on = e < ne;
        int32_t r = 0;
        if (on) {
            r = root[label[e]];
            label[e] = r;
            // a thread's edges ascend, so the first edge of a stretch under one root is the stretch's smallest: the others need not ask (the 16 M
            // edges of a giant block would otherwise all load the one word of its root)
            if ((n == 0 || r != cur) && vgl_load_agent(min_edge + r) > (uint32_t)e) atomicMin(min_edge + r, (uint32_t)e);
        }
        const bool turn = on && n > 0 && r != cur;
        bi_fetch_add_by_key(turn, cur, n, edges);
        if (turn) n = 0;
        if (on) { cur = r; n++; }
    }
    bi_fetch_add_by_key(n > 0, cur, n, edges);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_block_write(int32_t ne, int32_t *label, const uint32_t *min_edge)
{
    for (int64_t e = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; e < ne; e += (int64_t)gridDim.x * VGL_BLOCK) label[e] = (int32_t)min_edge[label[e]];
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_bicc_block_stats(int32_t V, const int32_t *edges, bi_cnt *cnt)
{
    int64_t blocks = 0;
    bi_cnt largest = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        const int32_t n = edges[v];
        blocks += n > 0;
        largest = max(largest, (bi_cnt)max(n, 0));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, __shfl_xor(largest, o));
    if (vgl_lane() == 0 && largest) atomicMax(cnt + BI_LARGEST, largest);
    vgl_wave_flush_add(cnt + BI_BLOCKS, blocks);
}

int bi_validate(const char *who, vgl_hip_ctx *c, vgl_hip_graph *g)
{
    static thread_local std::string msg;
    if (!c || !g) { msg = std::string(who) + ": null argument"; VGL_FAIL(msg.c_str()); }
    if (g->row_begin != 0 || g->row_end != g->V) { msg = std::string(who) + ": graph handle must own all rows (biconnectivity has no sharded form)"; VGL_FAIL(msg.c_str()); }
    return 0;
}

struct bi_level { int64_t off[VGL_RC_N]; int32_t n[VGL_RC_N]; };

}  // namespace

extern "C" {

int vgl_hip_bicc_prepare(vgl_hip_ctx *c, vgl_hip_graph *g, int64_t *undirected_edges)
{
    VGL_TRY(bi_validate("bicc_prepare", c, g));
    const vgl_simple_cache *sg = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_edge_ids(c, g, &sg, &built));
    VGL_HIP_TRY(hipStreamSynchronize(c->stream));
    if (undirected_edges) *undirected_edges = sg->ne;
    return 0;
}

int vgl_hip_bicc_run(vgl_hip_ctx *c, vgl_hip_graph *g, int32_t *d_edge_u, int32_t *d_edge_v, uint8_t *d_bridge, int32_t *d_edge_component, uint8_t *d_articulation,
                     int32_t *d_two_edge_component, vgl_hip_bicc_stats *stats)
{
    // every refusal comes before the first write to an output
    VGL_TRY(bi_validate("bicc_run", c, g));
    if (!d_edge_u && !d_edge_v && !d_bridge && !d_edge_component && !d_articulation && !d_two_edge_component)
        VGL_FAIL("bicc_run: all outputs are NULL (give at least one of d_edge_u / d_edge_v, d_bridge, d_edge_component, d_articulation, d_two_edge_component)");
    if ((d_edge_u == nullptr) != (d_edge_v == nullptr)) VGL_FAIL("bicc_run: d_edge_u and d_edge_v go together (both or neither)");
    const vgl_simple_cache *sg = nullptr;
    bool built = false;
    VGL_TRY(vgl_simple_ensure_edge_ids(c, g, &sg, &built));
    const int32_t V = g->V;
    const int32_t ne = (int32_t)sg->ne;
    const int64_t nnz = sg->csr.nnz;
    hipStream_t st = c->stream;
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_BICC_SHORT", "VGL_BICC_WAVE");
    const bool blocks = d_edge_component || d_articulation;
    vgl_hip_bicc_stats out;
    memset(&out, 0, sizeof(out));
    out.prepared_now = built ? 1 : 0;
    out.undirected_edges = ne;
    if (!blocks) out.articulation_points = out.biconnected_components = out.largest_component_edges = -1;
    if (V <= 0) {
        VGL_HIP_TRY(hipStreamSynchronize(st));
        if (stats) *stats = out;
        return 0;
    }
    const unsigned grid_v = vgl_grid(V, VGL_BLOCK, BI_MAX_GRID), grid_e = vgl_grid(ne, VGL_BLOCK, BI_MAX_GRID);

    // ---- scratch of the call, all of it drawn before the level loop ----
    // Plain hipMalloc blocks, not the stream-ordered pool.  With pooled blocks the SECOND run of a process on RMAT-20 refused in about one invocation in
    // three: a level's expansion read a list that was partly not what the launch before it had appended (504 467 listed vertices found 4 911 new ones
    // where 155 530 were due), and the check on the list tails fired.  An A/B on that graph (10 process starts of 3 runs each per side): pooled blocks
    // refused, with and without the agent-scope pre-check of the claim; plain blocks never did.  It is the second time a block handed back to the pool
    // and drawn again has not held up under kernels on this runtime (vgl_hip_internal.h: large blocks left the pool for that reason); DESIGN section 20.
    vgl_dev<bi_cnt> cnt;
    vgl_dev<int32_t> uf, level, parent, size, cursor, pre, low, high, lists, uf_block, edges_of, label_own;
    vgl_dev<uint32_t> min_edge;
    VGL_TRY(cnt.alloc(BI_NCNT));
    VGL_TRY(uf.alloc((size_t)V));
    VGL_TRY(level.alloc((size_t)V));
    VGL_TRY(parent.alloc((size_t)V));
    VGL_TRY(size.alloc((size_t)V));
    VGL_TRY(cursor.alloc((size_t)V));
    VGL_TRY(pre.alloc((size_t)V));
    VGL_TRY(low.alloc((size_t)V));
    VGL_TRY(high.alloc((size_t)V));
    VGL_TRY(lists.alloc((size_t)V));
    if (blocks) {
        VGL_TRY(uf_block.alloc((size_t)V));
        VGL_TRY(edges_of.alloc((size_t)V));
        VGL_TRY(min_edge.alloc((size_t)V));
        if (!d_edge_component) VGL_TRY(label_own.alloc((size_t)ne));
    }
    int32_t *label = d_edge_component ? d_edge_component : label_own.p;
    VGL_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(bi_cnt) * BI_NCNT, st));
    auto read = [&]() -> int { return vgl_publish_counters(c, "bicc_publish", cnt, BI_NCNT); };

    // ---- the classes, the roots ----
    {
        vgl_timed_launch tl(c, "bicc_classify");
        hipLaunchKernelGGL(vgl_k_bicc_init, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)sg->csr.deg.p, b, uf.p, level.p, size.p, cursor.p, cnt.p);
    }
    {
        vgl_timed_launch tl(c, "bicc_roots");
        hipLaunchKernelGGL(vgl_k_bicc_unite_edges, dim3(grid_e), dim3(VGL_BLOCK), 0, st, ne, (const int32_t *)sg->eu.p, (const int32_t *)sg->ev.p, uf.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(read());
    bi_lists L;
    int64_t cap[VGL_RC_N];
    {
        int64_t off = 0;
        for (int k = 0; k < VGL_RC_N; k++) {
            const int64_t rows = c->h_counters[BI_ROWS + k];
            if (rows < 0 || rows > V) VGL_FAIL("bicc_run: internal error (more rows in a class than vertices)");
            L.rows[k] = lists.p + off;
            L.cap[k] = (int32_t)rows;
            cap[k] = rows;
            off += rows;
        }
        if (off != V) VGL_FAIL("bicc_run: internal error (the row classes do not add up to the vertices)");
    }
    {
        vgl_timed_launch tl(c, "bicc_seed");
        hipLaunchKernelGGL(vgl_k_bicc_seed, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)uf.p, (const int32_t *)sg->csr.deg.p, b, level.p, parent.p, L, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(read());
    const int64_t components = c->h_counters[BI_ROOTS];

    // ---- the BFS: one host read per level ----
    bi_bfs t;
    t.rowptr = sg->csr.rowptr; t.adj = sg->csr.adj; t.deg = sg->csr.deg; t.level = level; t.parent = parent; t.L = L; t.cnt = cnt; t.b = b;
    std::vector<bi_level> levels;
    const char *const bfs_slot[VGL_RC_N] = {"bicc_bfs_short", "bicc_bfs_wave", "bicc_bfs_wg"};
    const char *const list_msg = "bicc_run: internal error (a class list longer than its class)";
    const int64_t grid_cap[VGL_RC_N] = {BI_MAX_GRID, BI_MAX_GRID, BI_MAX_GRID};
    vgl_rc_window w;                             // the level: [head, tail) of the cumulative class lists
    VGL_TRY(w.advance(c->h_counters + BI_TAIL, cap, list_msg));
    for (;;) {
        bi_level lv;
        for (int k = 0; k < VGL_RC_N; k++) {
            lv.off[k] = w.head[k];
            lv.n[k] = (int32_t)w.n(k);
        }
        const int64_t total = w.live();
        if (total == 0) break;
        if ((int64_t)levels.size() >= V) VGL_FAIL("bicc_run: internal error (more levels than vertices)");
        levels.push_back(lv);
        t.next_level = (int32_t)levels.size();
        const int32_t *const rows[VGL_RC_N] = {L.rows[0] + w.head[0], L.rows[1] + w.head[1], L.rows[2] + w.head[2]};
        VGL_TRY(vgl_rc_launch_trio(c, bfs_slot, w, grid_cap, vgl_k_bicc_bfs<VGL_RC_SHORT>, vgl_k_bicc_bfs<VGL_RC_WAVE>, vgl_k_bicc_bfs<VGL_RC_WG>, rows, t));
        VGL_TRY(read());
        VGL_TRY(w.advance(c->h_counters + BI_TAIL, cap, list_msg));
    }
    if (w.total() != V) {
        static thread_local std::string msg;
        msg = "bicc_run: internal error (the forest does not reach every vertex): " + std::to_string(w.head[0]) + " + " + std::to_string(w.head[1]) + " + " + std::to_string(w.head[2]) + " of " +
              std::to_string(V) + " listed in " + std::to_string(levels.size()) + " levels from " + std::to_string(components) + " roots; the classes hold " + std::to_string(L.cap[0]) + ", " +
              std::to_string(L.cap[1]) + ", " + std::to_string(L.cap[2]) + "; listed per level:";
        for (const bi_level &lv : levels) msg += " " + std::to_string((int64_t)lv.n[0] + lv.n[1] + lv.n[2]);
        VGL_FAIL(msg.c_str());
    }
    const int32_t depth = (int32_t)levels.size();
    auto slice_of = [&](const bi_level &lv) {
        bi_slice s;
        for (int k = 0; k < VGL_RC_N; k++) { s.rows[k] = L.rows[k] + lv.off[k]; s.n[k] = lv.n[k]; }
        return s;
    };
    auto grid_of = [&](const bi_level &lv) { return dim3(vgl_grid((int64_t)lv.n[0] + lv.n[1] + lv.n[2], VGL_BLOCK, BI_MAX_GRID)); };

    // ---- subtree intervals ----
    for (int32_t l = depth - 1; l >= 1; l--) {
        vgl_timed_launch tl(c, "bicc_size");
        hipLaunchKernelGGL(vgl_k_bicc_size, grid_of(levels[(size_t)l]), dim3(VGL_BLOCK), 0, st, slice_of(levels[(size_t)l]), (const int32_t *)parent.p, size.p);
    }
    for (int32_t l = 0; l < depth; l++) {
        vgl_timed_launch tl(c, "bicc_pre");
        hipLaunchKernelGGL(vgl_k_bicc_pre, grid_of(levels[(size_t)l]), dim3(VGL_BLOCK), 0, st, slice_of(levels[(size_t)l]), l == 0 ? 1 : 0, (const int32_t *)parent.p, (const int32_t *)size.p, cursor.p,
                           pre.p, cnt.p + BI_TREES);
    }
    VGL_HIP_TRY(hipGetLastError());

    // ---- low / high: the rows by class, then the levels ----
    const char *const local_slot[VGL_RC_N] = {"bicc_local_short", "bicc_local_wave", "bicc_local_wg"};
    const char *const art_slot[VGL_RC_N] = {"bicc_art_short", "bicc_art_wave", "bicc_art_wg"};
    auto rows_by_class = [&](auto op, const char *const *slot) -> int {
        using OP = decltype(op);
        const int32_t *const rows[VGL_RC_N] = {L.rows[0], L.rows[1], L.rows[2]};
        return vgl_rc_launch_trio(c, slot, cap, grid_cap, vgl_k_bicc_rows<VGL_RC_SHORT, OP>, vgl_k_bicc_rows<VGL_RC_WAVE, OP>, vgl_k_bicc_rows<VGL_RC_WG, OP>, rows, op);
    };
    {
        bi_local_op op;
        op.rowptr = sg->csr.rowptr; op.adj = sg->csr.adj; op.parent = parent; op.pre = pre; op.low = low; op.high = high;
        VGL_TRY(rows_by_class(op, local_slot));
    }
    for (int32_t l = depth - 1; l >= 1; l--) {
        vgl_timed_launch tl(c, "bicc_lowhigh");
        hipLaunchKernelGGL(vgl_k_bicc_lowhigh, grid_of(levels[(size_t)l]), dim3(VGL_BLOCK), 0, st, slice_of(levels[(size_t)l]), (const int32_t *)parent.p, low.p, high.p);
    }
    VGL_HIP_TRY(hipGetLastError());

    // ---- per edge: bridges, and the unions of the blocks and of the 2-edge-connected components ----
    if (d_edge_u && ne > 0) {
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_u, sg->eu, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
        VGL_HIP_TRY(hipMemcpyAsync(d_edge_v, sg->ev, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToDevice, st));
    }
    int32_t *const uf_two = d_two_edge_component ? uf.p : nullptr;   // the roots' union-find has done its work: its array serves again
    if (uf_two || blocks) {
        vgl_timed_launch tl(c, "bicc_reset");
        hipLaunchKernelGGL(vgl_k_bicc_reset, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, uf_two, blocks ? uf_block.p : nullptr, blocks ? edges_of.p : nullptr, blocks ? min_edge.p : nullptr);
    }
    {
        bi_edge te;
        te.eu = sg->eu; te.ev = sg->ev; te.parent = parent; te.pre = pre; te.size = size; te.low = low; te.high = high;
        te.bridge = d_bridge; te.name = blocks ? label : nullptr; te.uf_block = blocks ? uf_block.p : nullptr; te.uf_two = uf_two; te.cnt = cnt;
        vgl_timed_launch tl(c, "bicc_edge");
        hipLaunchKernelGGL(vgl_k_bicc_edge, dim3(grid_e), dim3(VGL_BLOCK), 0, st, ne, te);
    }
    VGL_HIP_TRY(hipGetLastError());
    if (blocks) {
        int32_t *const root_of = cursor;                              // (the preorder is done with it)
        {
            vgl_timed_launch tl(c, "bicc_flatten");
            hipLaunchKernelGGL(vgl_k_bicc_flatten, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, uf_block.p, root_of, (bi_cnt *)nullptr);
        }
        {
            vgl_timed_launch tl(c, "bicc_block");
            hipLaunchKernelGGL(vgl_k_bicc_block_min, dim3(grid_e), dim3(VGL_BLOCK), 0, st, ne, label, (const int32_t *)root_of, min_edge.p, edges_of.p);
        }
        {
            vgl_timed_launch tl(c, "bicc_block");
            hipLaunchKernelGGL(vgl_k_bicc_block_write, dim3(grid_e), dim3(VGL_BLOCK), 0, st, ne, label, (const uint32_t *)min_edge.p);
        }
        {
            vgl_timed_launch tl(c, "bicc_block");
            hipLaunchKernelGGL(vgl_k_bicc_block_stats, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)edges_of.p, cnt.p);
        }
        bi_art_op op;
        op.rowptr = sg->csr.rowptr; op.eid = sg->eid; op.label = label; op.art = d_articulation; op.cnt = cnt;
        VGL_TRY(rows_by_class(op, art_slot));
    }
    if (d_two_edge_component) {                                       // (a flatten too, under the name of its pass)
        vgl_timed_launch tl(c, "bicc_twoecc");
        hipLaunchKernelGGL(vgl_k_bicc_flatten, dim3(grid_v), dim3(VGL_BLOCK), 0, st, V, uf_two, d_two_edge_component, cnt.p + BI_TWOECC);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(read());
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.components = components;
    out.bridges = c->h_counters[BI_BRIDGES];
    out.two_edge_components = components + out.bridges;              // every bridge cuts one component in two
    if (d_two_edge_component && c->h_counters[BI_TWOECC] != out.two_edge_components)
        VGL_FAIL("bicc_run: internal error (the 2-edge-connected components do not number components + bridges)");
    if (c->h_counters[BI_TREES] != V) {
        static thread_local std::string msg;
        msg = "bicc_run: internal error (the trees' sizes do not add up to the vertices): " + std::to_string(c->h_counters[BI_TREES]) + " of " + std::to_string(V) + ", " +
              std::to_string(components) + " roots, depth " + std::to_string(depth);
        VGL_FAIL(msg.c_str());
    }
    if (blocks) {
        out.articulation_points = c->h_counters[BI_ARTS];
        out.biconnected_components = c->h_counters[BI_BLOCKS];
        out.largest_component_edges = c->h_counters[BI_LARGEST];
    }
    out.depth = depth;
    // the model, a lower bound in V, E', nnz = 2 E' and depth alone
    out.algorithmic_bytes = 92 * (int64_t)V + 16 * nnz + 24 * (int64_t)ne + 8 * BI_NCNT * ((int64_t)depth + 1) + (d_edge_u ? 16 * (int64_t)ne : 0) + (d_bridge ? (int64_t)ne : 0) +
                            (blocks ? 33 * (int64_t)V + 20 * (int64_t)ne + 8 * nnz : 0) + (d_two_edge_component ? 12 * (int64_t)V : 0);
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
