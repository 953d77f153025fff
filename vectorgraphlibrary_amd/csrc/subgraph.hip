// subgraph.hip -- subgraph extraction (a stable filter of adjacency rows under a vertex mask and / or an entry mask), bounded multi-seed reach (k-hop)
// and fixed-fanout neighbour sampling without replacement.  The contract is written out in include/vgl_hip.h; DESIGN section 24 has the kernels, their
// bounds and the bytes models.
//
// Filter plan: an exclusive scan of the vertex mask (vgl_prim.h) and a pass that marks the dropped vertices give new_id; the kept rows are counted
// and listed per row class (vgl_rowclass.h: short 8 lanes per row, wave, workgroup) and per direction; one counting kernel per class writes the
// number of surviving entries of every kept row, and the same scan turns the counts into the new int64 rowptr.  Two reads of the pinned counter
// mirror (sizes of the lists; V', E'out, E'in) and one stream synchronise at the end.
//
// Fill: the counting kernels again, now writing.  The compaction is ORDERED: every row has one owner (an 8-lane group, a wavefront, a workgroup),
// the position of a survivor is the row's new start + the survivors of the chunks before (a running base in a register) + the survivors before it
// in its chunk (ballot and popcount of the lanes below; the workgroup adds an LDS scan over its four wavefronts).  No atomic touches an output.
//
// k-hop: seeds validated, then marked 0 in a level array of -1; level-synchronous top-down steps (vgl_hip_bfs_step_top_down on the handle, on the
// cached transposed handle, or on both) until `hops` levels were expanded or a frontier is empty.
//
// Sampling: key(p, seed) is a function of the position alone, so selection reads no memory.  Short and wave rows rank-count (an entry is taken when
// fewer than `fanout` entries of its row have a smaller key); workgroup rows find the fanout-th smallest key by a 4 x 8-bit radix select over
// recomputed keys (LDS histograms).  The emit is the ordered compaction of the filter.
#include "vgl_rowclass.h"
#include "vgl_prim.h"
#include <cstring>
#include <algorithm>

struct vgl_hip_subgraph_plan {
    vgl_hip_graph *g = nullptr;
    int32_t V = 0, Vk = 0;
    bool planned[2] = {false, false};
    const uint8_t *keep_entry = nullptr;         // borrowed until the fill (direction 0 only)
    vgl_dev<int32_t> new_id, old_id, lists;      // V (+ 1: V', where the scan ends); V'; the kept rows (parent ids) per direction and class
    vgl_dev<int64_t> rowptr[2];                  // V' + 1 each
    int64_t rows[2][VGL_RC_N] = {{0, 0, 0}, {0, 0, 0}}, off[2][VGL_RC_N] = {{0, 0, 0}, {0, 0, 0}};
    vgl_hip_subgraph_stats st;
};

namespace {

constexpr int64_t SUB_MAX_GRID = 2048;           // workgroups of a grid-stride kernel
enum {
    SUB_VK = 0,         // kept vertices
    SUB_ROWS = 1,       // + 3 * direction + class: kept rows per class
    SUB_READ = 7,       // + direction: full lengths of the kept rows
    SUB_KEPT = 9,       // + direction: surviving entries
    SUB_TAIL = 11,      // + 3 * direction + class: rows appended to the class list so far
    SUB_NCNT = 17
};
enum {
    SMP_TAIL = 0,       // + class: rows appended to the class list so far
    SMP_ROWS = 3,       // + class: seeds per class
    SMP_BAD = 6,        // seeds outside [0, V)
    SMP_EXAM = 7,       // sum of the seeds' degrees
    SMP_TOTAL = 8,      // sampled entries
    SMP_NCNT = 9
};
enum { KH_BAD = 0, KH_REACHED = 1, KH_NCNT = 2 };
static_assert(SUB_NCNT <= C_NSLOTS && SMP_NCNT <= C_NSLOTS, "the counters are mirrored in the context's pinned slots");

bool sub_sharded(const vgl_hip_graph *g) { return g->row_begin != 0 || g->row_end != g->V; }

// ---- new_id: the exclusive scan of the vertex mask (nullptr: every vertex is kept), then -1 for the dropped vertices ----
struct sub_keep_src {           // element v of the scan's input; element V is 0, so that the scan's last output is the number of kept vertices
    const uint8_t *keep; int32_t V;
    __device__ __forceinline__ int32_t operator()(int64_t v) const { return v < V && (!keep || keep[v] != 0); }
};
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sub_drop(int32_t V, const uint8_t *keep, int32_t *new_id)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK)
        if (keep[v] == 0) new_id[v] = -1;
}

// ---- the kept rows per direction and class ----
struct sub_rows_src {
    int32_t V;
    const int32_t *new_id;
    const int64_t *rowptr[2];    // nullptr: the direction is not planned
    vgl_rc_bounds b;
};
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sub_classify(sub_rows_src s, unsigned long long *cnt)
{
    int64_t rows[2][VGL_RC_N] = {{0, 0, 0}, {0, 0, 0}}, read[2] = {0, 0};
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < s.V; v += (int64_t)gridDim.x * VGL_BLOCK) {
        if (s.new_id[v] < 0) continue;
#pragma unroll
        for (int d = 0; d < 2; d++)
            if (s.rowptr[d]) {
                const int64_t len = s.rowptr[d][v + 1] - s.rowptr[d][v];
                const int k = vgl_rc_class_of(len, s.b);
#pragma unroll
                for (int q = 0; q < VGL_RC_N; q++) rows[d][q] += k == q;
                read[d] += len;
            }
    }
#pragma unroll
    for (int d = 0; d < 2; d++) {
#pragma unroll
        for (int q = 0; q < VGL_RC_N; q++) vgl_wave_flush_add(cnt + SUB_ROWS + 3 * d + q, rows[d][q]);
        vgl_wave_flush_add(cnt + SUB_READ + d, read[d]);
    }
}
struct sub_lists { vgl_rc_bounded l[2][VGL_RC_N]; };
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sub_lists(sub_rows_src s, sub_lists L, int32_t *old_id, unsigned long long *tail)
{
    vgl_rc_stage st[2 * VGL_RC_N];
    vgl_rc_stage_open(st);
    for (int64_t base = (int64_t)blockIdx.x * VGL_BLOCK; base < s.V; base += (int64_t)gridDim.x * VGL_BLOCK) {      // (uniform over the workgroup)
        const int64_t v = base + threadIdx.x;
        const int32_t nid = v < s.V ? s.new_id[v] : -1;
        if (nid >= 0) old_id[nid] = (int32_t)v;
#pragma unroll
        for (int d = 0; d < 2; d++) {
            if (!s.rowptr[d]) continue;                               // (uniform)
            const int k = nid >= 0 ? vgl_rc_class_of(s.rowptr[d][v + 1] - s.rowptr[d][v], s.b) : -1;
#pragma unroll
            for (int q = 0; q < VGL_RC_N; q++) st[3 * d + q].keep(k == q, (int32_t)v, L.l[d][q], tail + 3 * d + q);
        }
    }
#pragma unroll
    for (int d = 0; d < 2; d++)
#pragma unroll
        for (int q = 0; q < VGL_RC_N; q++) st[3 * d + q].flush(L.l[d][q], tail + 3 * d + q);
}

// ---- the filter: FILL = false counts the survivors of every listed row, FILL = true writes them in their stored order ----
struct sub_dir {
    const int64_t *rowptr;       // the parent's, of this direction
    const int32_t *adj;
    const int32_t *new_id;
    const uint8_t *keep_entry;   // nullptr: every entry is kept (always nullptr for direction 1)
    // does entry e survive, and under which id does its far end
    __device__ __forceinline__ bool keep(int64_t e, int32_t &far) const
    {
        far = new_id[adj[e]];
        return far >= 0 && (!keep_entry || keep_entry[e] != 0);
    }
};
struct sub_out {
    int64_t *count;              // counting: by new id
    const int64_t *rowptr;       // filling: the new row starts; a position at or past the row's new end is never stored to
    int32_t *adj;
    int64_t *origin;             // may be nullptr
};
// the listed row i: its first entry, its length, its new id
struct sub_row { int64_t s, len; int32_t nid; };
__device__ __forceinline__ sub_row sub_row_of(const sub_dir &a, const int32_t *list, int64_t i, int64_t n)
{
    if (i >= n) return sub_row{0, 0, 0};
    const int32_t v = list[i];
    const int64_t s = a.rowptr[v];
    return sub_row{s, a.rowptr[v + 1] - s, a.new_id[v]};
}
template <int CLS, bool FILL>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sub(const int32_t *list, int32_t n, sub_dir a, sub_out o)
{
    using T = vgl_rc_team<CLS>;
    for (int64_t at0 = T::begin(); at0 < n; at0 += T::stride()) {
        const int64_t i = T::item(at0);
        const bool has = i < n;
        const sub_row r = sub_row_of(a, list, i, n);
        const int64_t at = FILL && has ? o.rowptr[r.nid] : 0, end = FILL && has ? o.rowptr[r.nid + 1] : 0;
        int64_t kept = 0;                                             // survivors of the chunks before: the running base
        for (int64_t j0 = 0; T::together(j0 < r.len); j0 += T::LANES) {
            const int64_t e = r.s + j0 + T::lane();
            int32_t far = -1;
            const bool k = j0 + T::lane() < r.len && a.keep(e, far);
            int tot = 0;
            const int rank = T::rank(k, &tot);
            if (FILL && k) {
                const int64_t pos = at + kept + rank;
                if (pos < end) {
                    o.adj[pos] = far;
                    if (o.origin) o.origin[pos] = e;
                }
            }
            kept += tot;
        }
        if (!FILL && T::lead() && has) o.count[r.nid] = kept;
    }
}
const int64_t sub_grid_cap[VGL_RC_N] = {4 * SUB_MAX_GRID, 4 * SUB_MAX_GRID, 4 * SUB_MAX_GRID};
template <bool FILL>
int sub_launch(vgl_hip_ctx *c, const vgl_hip_subgraph_plan *p, int d, const sub_dir &a, const sub_out &o)
{
    const char *const count_slot[VGL_RC_N] = {"sub_count_short", "sub_count_wave", "sub_count_wg"};
    const char *const fill_slot[VGL_RC_N] = {"sub_fill_short", "sub_fill_wave", "sub_fill_wg"};
    const int32_t *const list[VGL_RC_N] = {p->lists.p + p->off[d][0], p->lists.p + p->off[d][1], p->lists.p + p->off[d][2]};
    return vgl_rc_launch_trio(c, FILL ? fill_slot : count_slot, p->rows[d], sub_grid_cap, vgl_k_sub<VGL_RC_SHORT, FILL>, vgl_k_sub<VGL_RC_WAVE, FILL>, vgl_k_sub<VGL_RC_WG, FILL>, list, a, o);
}
sub_dir sub_dir_of(const vgl_hip_subgraph_plan *p, int d)
{
    const vgl_dir_csr &csr = d == 0 ? p->g->out : p->g->in;
    return sub_dir{csr.rowptr, csr.adj, p->new_id.p, d == 0 ? p->keep_entry : nullptr};
}

// ---- k-hop ----
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_khop_check(int32_t V, const int32_t *seeds, int64_t n, unsigned long long *cnt)
{
    int64_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) bad += seeds[i] < 0 || seeds[i] >= V;
    vgl_wave_flush_add(cnt + KH_BAD, bad);
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_khop_seed(const int32_t *seeds, int64_t n, int32_t *hop)
{
    for (int64_t i = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VGL_BLOCK) hop[seeds[i]] = 0;      // (repeats store the same value)
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_khop_fill(int32_t V, int32_t *hop)
{
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) hop[v] = -1;
}
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_khop_reached(int32_t V, const int32_t *hop, unsigned long long *cnt)
{
    int64_t r = 0;
    for (int64_t v = (int64_t)blockIdx.x * VGL_BLOCK + threadIdx.x; v < V; v += (int64_t)gridDim.x * VGL_BLOCK) r += hop[v] >= 0;
    vgl_wave_flush_add(cnt + KH_REACHED, r);
}

// ---- sampling ----
// item i is seed i: its class by its degree; a counting pass (count != nullptr) also stores count[i] = min(fanout, degree), 0 for a seed out of range
struct smp_src {
    int32_t V;
    const int64_t *rowptr;
    const int32_t *seeds;
    int32_t fanout;
    vgl_rc_bounds b;
    int64_t *count;
    __device__ __forceinline__ int cls(int64_t i, int64_t &work) const
    {
        const int32_t v = seeds[i];
        const bool in = v >= 0 && v < V;
        if (in) work = rowptr[v + 1] - rowptr[v];
        if (count) count[i] = work < fanout ? work : fanout;
        return in ? vgl_rc_class_of(work, b) : -1;
    }
};
struct smp_args {
    const int64_t *rowptr;       // of the sampled direction
    const int32_t *adj;
    const int32_t *seeds;
    const int64_t *out_rowptr;
    int32_t *out_adj;
    int64_t *out_origin;         // may be nullptr
    int32_t fanout;
    uint32_t mix;                // fmix32(seed + 0x9e3779b9)
    __device__ __forceinline__ uint32_t key(int64_t p) const { return vgl_fmix32((uint32_t)p ^ mix); }
};
struct smp_row { int64_t s, len, at, end; };      // the row's entries; its slots [at, end) of the output, never stored past
__device__ __forceinline__ smp_row smp_row_of(const smp_args &a, const int32_t *list, int64_t i, int64_t n)
{
    if (i >= n) return smp_row{0, 0, 0, 0};
    const int32_t r = list[i], v = a.seeds[r];
    const int64_t s = a.rowptr[v];
    return smp_row{s, a.rowptr[v + 1] - s, a.out_rowptr[r], a.out_rowptr[r + 1]};
}
// short and wave rows: an entry is taken when fewer than fanout entries of the row have a smaller key
template <int CLS>
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sample_group(const int32_t *list, int32_t n, smp_args a)
{
    using T = vgl_rc_team<CLS>;
    static_assert(CLS != VGL_RC_WG, "workgroup rows select by radix (vgl_k_sample_wg)");
    for (int64_t at = T::begin(); at < n; at += T::stride()) {
        const smp_row r = smp_row_of(a, list, T::item(at), n);
        const bool all = r.len <= a.fanout;
        int64_t kept = 0;
        for (int64_t j0 = 0; T::together(j0 < r.len); j0 += T::LANES) {
            const int64_t j = j0 + T::lane();
            bool k = j < r.len;
            if (k && !all) {
                const uint32_t mine = a.key(r.s + j);
                int32_t rank = 0;
                for (int64_t t = 0; t < r.len && rank < a.fanout; t++) rank += a.key(r.s + t) < mine;
                k = rank < a.fanout;
            }
            int tot = 0;
            const int before = T::rank(k, &tot);
            if (k) {
                const int64_t pos = r.at + kept + before;
                if (pos < r.end) {
                    a.out_adj[pos] = a.adj[r.s + j];
                    if (a.out_origin) a.out_origin[pos] = r.s + j;
                }
            }
            kept += tot;
        }
    }
}
// a workgroup per row: the fanout-th smallest key by four 8-bit radix passes (most significant byte first), then every entry whose key is not larger
__global__ __launch_bounds__(VGL_BLOCK) void vgl_k_sample_wg(const int32_t *list, int32_t n, smp_args a)
{
    __shared__ unsigned s_hist[256];
    __shared__ int64_t s_scan[VGL_WAVES];
    __shared__ unsigned s_bin, s_k;
    static_assert(VGL_BLOCK == 256, "one histogram bin per thread");
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {             // (uniform over the workgroup)
        const smp_row r = smp_row_of(a, list, i, n);
        uint32_t limit = 0xffffffffu;                                 // the largest key taken
        if (r.len > a.fanout) {                                       // (uniform)
            uint32_t prefix = 0;
            unsigned want = (unsigned)a.fanout;                       // the rank sought among the keys that share the prefix, from 1
            for (int pass = 0; pass < 4; pass++) {
                const int shift = 24 - 8 * pass;
                __syncthreads();                                      // s_bin / s_k / the histogram of the pass before have been read
                s_hist[threadIdx.x] = 0;
                __syncthreads();
                for (int64_t j = threadIdx.x; j < r.len; j += VGL_BLOCK) {
                    const uint32_t key = a.key(r.s + j);
                    if (((uint64_t)key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                const int64_t h = s_hist[threadIdx.x];
                int64_t tot = 0;
                const int64_t ex = vgl_block_excl_add(h, s_scan, &tot);
                if (ex < (int64_t)want && (int64_t)want <= ex + h) { s_bin = threadIdx.x; s_k = (unsigned)((int64_t)want - ex); }
                __syncthreads();
                prefix = (prefix << 8) | s_bin;
                want = s_k;
            }
            limit = prefix;
        }
        int64_t kept = 0;
        for (int64_t j0 = 0; j0 < r.len; j0 += VGL_BLOCK) {
            const int64_t j = j0 + threadIdx.x;
            const bool k = j < r.len && a.key(r.s + j) <= limit;
            int tot = 0;
            const int rank = vgl_rc_team<VGL_RC_WG>::rank(k, &tot);
            if (k) {
                const int64_t pos = r.at + kept + rank;
                if (pos < r.end) {
                    a.out_adj[pos] = a.adj[r.s + j];
                    if (a.out_origin) a.out_origin[pos] = r.s + j;
                }
            }
            kept += tot;
        }
    }
}

}  // namespace

extern "C" {

int vgl_hip_subgraph_plan_create(vgl_hip_ctx *c, vgl_hip_graph *g, const uint8_t *d_keep_vertex, const uint8_t *d_keep_entry, vgl_hip_subgraph_plan **out)
{
    if (!c || !g || !out) VGL_FAIL("subgraph_plan_create: null argument");
    if (sub_sharded(g)) VGL_FAIL("subgraph_plan_create: graph handle must own all rows (subgraph extraction has no sharded form)");
    if (!d_keep_vertex && !d_keep_entry) VGL_FAIL("subgraph_plan_create: both masks are NULL (give at least one of d_keep_vertex, d_keep_entry)");
    const int32_t V = g->V;
    hipStream_t st = c->stream;
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_SUB_SHORT", "VGL_SUB_WAVE");
    vgl_building<vgl_hip_subgraph_plan> p(new vgl_hip_subgraph_plan(), vgl_synced_delete<vgl_hip_subgraph_plan>{c});
    p->g = g;
    p->V = V;
    p->keep_entry = d_keep_entry;
    p->planned[0] = true;
    p->planned[1] = g->in.rowptr != nullptr && !d_keep_entry;
    memset(&p->st, 0, sizeof(p->st));

    vgl_dev<unsigned long long> cnt;
    vgl_scratch tmp;                                                  // of the scans
    VGL_TRY(vgl_open_counters(c, &cnt, SUB_NCNT));
    VGL_TRY(p->new_id.alloc(st, (size_t)V + 1));
    const auto kept = vgl_computed(sub_keep_src{d_keep_vertex, V});
    VGL_TRY(vgl_exclusive_scan(c, tmp, kept, p->new_id.p, (size_t)V + 1, VGL_SIZE_ONLY));
    {
        vgl_timed_launch tl(c, "sub_scan");
        VGL_TRY(vgl_exclusive_scan(c, tmp, kept, p->new_id.p, (size_t)V + 1));
    }
    VGL_HIP_TRY(hipMemcpyAsync(cnt.p + SUB_VK, p->new_id.p + V, sizeof(int32_t), hipMemcpyDeviceToDevice, st));      // (the slot's upper half stays 0)
    if (d_keep_vertex) {
        vgl_timed_launch tl(c, "sub_scan");
        hipLaunchKernelGGL(vgl_k_sub_drop, dim3(vgl_grid(V, VGL_BLOCK, SUB_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, d_keep_vertex, p->new_id.p);
    }
    const sub_rows_src src{V, p->new_id.p, {g->out.rowptr, p->planned[1] ? g->in.rowptr : nullptr}, b};
    {
        vgl_timed_launch tl(c, "sub_scan");
        hipLaunchKernelGGL(vgl_k_sub_classify, dim3(vgl_grid(V, VGL_BLOCK, SUB_MAX_GRID)), dim3(VGL_BLOCK), 0, st, src, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_publish_counters(c, "sub_publish", cnt, SUB_NCNT));
    const int64_t Vk = c->h_counters[SUB_VK];
    if (Vk < 0 || Vk > V) VGL_FAIL("subgraph_plan_create: internal error (the kept vertices exceed V)");
    p->Vk = (int32_t)Vk;
    int64_t at = 0;
    for (int d = 0; d < 2; d++) {
        int64_t total = 0;
        for (int k = 0; k < VGL_RC_N; k++) {
            p->rows[d][k] = c->h_counters[SUB_ROWS + 3 * d + k];
            p->off[d][k] = at;
            at += p->rows[d][k];
            total += p->rows[d][k];
        }
        if (total != (p->planned[d] ? Vk : 0)) VGL_FAIL("subgraph_plan_create: internal error (the classes do not add up to the kept rows)");
    }
    vgl_hip_subgraph_stats &s = p->st;
    s.vertices_kept = Vk;
    s.rows_short_out = p->rows[0][0]; s.rows_wave_out = p->rows[0][1]; s.rows_wg_out = p->rows[0][2];
    s.rows_short_in = p->rows[1][0]; s.rows_wave_in = p->rows[1][1]; s.rows_wg_in = p->rows[1][2];
    s.entries_read_out = c->h_counters[SUB_READ + 0];
    s.entries_read_in = c->h_counters[SUB_READ + 1];
    if (Vk > 0) {
        VGL_TRY(p->old_id.alloc(st, (size_t)Vk));
        VGL_TRY(p->lists.alloc(st, (size_t)at));
        sub_lists L;
        for (int d = 0; d < 2; d++)
            for (int k = 0; k < VGL_RC_N; k++) L.l[d][k] = vgl_rc_bounded{p->lists.p + p->off[d][k], (int32_t)p->rows[d][k]};
        {
            vgl_timed_launch tl(c, "sub_scan");
            hipLaunchKernelGGL(vgl_k_sub_lists, dim3(vgl_grid(V, VGL_BLOCK, SUB_MAX_GRID)), dim3(VGL_BLOCK), 0, st, src, L, p->old_id.p, cnt + SUB_TAIL);
        }
        VGL_HIP_TRY(hipGetLastError());
        for (int d = 0; d < 2; d++) {
            if (!p->planned[d]) continue;
            VGL_TRY(p->rowptr[d].alloc(st, (size_t)Vk + 1));
            VGL_HIP_TRY(hipMemsetAsync(p->rowptr[d].p + Vk, 0, sizeof(int64_t), st));      // (every other entry is written by its row's owner)
            VGL_TRY(sub_launch<false>(c, p.get(), d, sub_dir_of(p.get(), d), sub_out{p->rowptr[d].p, nullptr, nullptr, nullptr}));
            VGL_TRY(vgl_exclusive_scan(c, tmp, p->rowptr[d].p, p->rowptr[d].p, (size_t)Vk + 1, VGL_SIZE_ONLY));
            {
                vgl_timed_launch tl(c, "sub_scan");
                VGL_TRY(vgl_exclusive_scan(c, tmp, p->rowptr[d].p, p->rowptr[d].p, (size_t)Vk + 1));
            }
            VGL_HIP_TRY(hipMemcpyAsync(cnt.p + SUB_KEPT + d, p->rowptr[d].p + Vk, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        }
        VGL_TRY(vgl_publish_counters(c, "sub_publish", cnt, SUB_NCNT));
        s.entries_kept_out = c->h_counters[SUB_KEPT + 0];
        s.entries_kept_in = c->h_counters[SUB_KEPT + 1];
    }
    const int64_t me = d_keep_entry ? 1 : 0;
    s.algorithmic_bytes = (d_keep_vertex ? (int64_t)V : 0) + 4 * (int64_t)V + 4 * Vk;
    for (int d = 0; d < 2; d++)
        if (p->planned[d]) {
            const int64_t read = d == 0 ? s.entries_read_out : s.entries_read_in, kept = d == 0 ? s.entries_kept_out : s.entries_kept_in;
            s.algorithmic_bytes += 56 * Vk + 32 * (Vk + 1) + (16 + 2 * me) * read + 4 * kept;
        }
    VGL_HIP_TRY(hipStreamSynchronize(st));
    *out = p.release();
    return 0;
}

int vgl_hip_subgraph_plan_info(vgl_hip_subgraph_plan *p, int32_t *vertices, int64_t *out_entries, int64_t *in_entries, vgl_hip_subgraph_stats *stats)
{
    if (!p) VGL_FAIL("subgraph_plan_info: null argument");
    if (vertices) *vertices = p->Vk;
    if (out_entries) *out_entries = p->st.entries_kept_out;
    if (in_entries) *in_entries = p->planned[1] ? p->st.entries_kept_in : -1;
    if (stats) *stats = p->st;
    return 0;
}

int vgl_hip_subgraph_plan_vertex_maps(vgl_hip_ctx *c, vgl_hip_subgraph_plan *p, int32_t *d_new_id, int32_t *d_old_id)
{
    if (!c || !p) VGL_FAIL("subgraph_plan_vertex_maps: null argument");
    if (d_new_id && p->V > 0) VGL_HIP_TRY(hipMemcpyAsync(d_new_id, p->new_id.p, sizeof(int32_t) * (size_t)p->V, hipMemcpyDeviceToDevice, c->stream));
    if (d_old_id && p->Vk > 0) VGL_HIP_TRY(hipMemcpyAsync(d_old_id, p->old_id.p, sizeof(int32_t) * (size_t)p->Vk, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int vgl_hip_subgraph_plan_fill(vgl_hip_ctx *c, vgl_hip_subgraph_plan *p, int direction, int64_t *d_rowptr, int32_t *d_adj, int64_t *d_origin)
{
    if (!c || !p) VGL_FAIL("subgraph_plan_fill: null argument");
    if (direction != 0 && direction != 1) VGL_FAIL("subgraph_plan_fill: direction must be 0 (outgoing) or 1 (incoming)");
    if (!p->planned[direction])
        VGL_FAIL(p->keep_entry ? "subgraph_plan_fill: with an entry mask only direction 0 can be filled (transpose the result for its incoming CSR)"
                               : "subgraph_plan_fill: direction 1 needs the incoming CSR");
    const int64_t kept = direction == 0 ? p->st.entries_kept_out : p->st.entries_kept_in;
    if (p->Vk == 0) return 0;                                         // nothing to write
    if (!d_rowptr || (kept > 0 && !d_adj)) VGL_FAIL("subgraph_plan_fill: d_rowptr and d_adj must not be NULL");
    VGL_HIP_TRY(hipMemcpyAsync(d_rowptr, p->rowptr[direction].p, sizeof(int64_t) * ((size_t)p->Vk + 1), hipMemcpyDeviceToDevice, c->stream));
    if (kept == 0) return 0;
    return sub_launch<true>(c, p, direction, sub_dir_of(p, direction), sub_out{nullptr, p->rowptr[direction].p, d_adj, d_origin});
}

int vgl_hip_subgraph_plan_destroy(vgl_hip_ctx *c, vgl_hip_subgraph_plan *p)
{
    if (!c) VGL_FAIL("subgraph_plan_destroy: null argument");
    if (!p) return 0;
    (void)hipStreamSynchronize(c->stream);
    delete p;
    return 0;
}

int vgl_hip_khop_run(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *d_seeds, int64_t n, int32_t hops, int direction, int symmetric, int32_t *d_hop,
                     vgl_hip_khop_stats *stats)
{
    if (!c || !g) VGL_FAIL("khop_run: null argument");
    if (sub_sharded(g)) VGL_FAIL("khop_run: graph handle must own all rows (k-hop has no sharded form)");
    if (!d_hop) VGL_FAIL("khop_run: d_hop must not be NULL");
    if (n < 0) VGL_FAIL("khop_run: n is negative");
    if (n > 0 && !d_seeds) VGL_FAIL("khop_run: d_seeds must not be NULL");
    if (hops < 0) VGL_FAIL("khop_run: hops is negative");
    if (direction != 0 && direction != 1) VGL_FAIL("khop_run: direction must be 0 (outgoing) or 1 (incoming)");
    if ((symmetric || direction == 1) && !g->in.rowptr) VGL_FAIL(symmetric ? "khop_run: symmetric needs the incoming CSR" : "khop_run: direction 1 needs the incoming CSR");
    const int32_t V = g->V;
    hipStream_t st = c->stream;
    vgl_hip_khop_stats out;
    memset(&out, 0, sizeof(out));
    vgl_dev<unsigned long long> cnt;
    VGL_TRY(vgl_open_counters(c, &cnt, KH_NCNT));
    if (n > 0) {
        {
            vgl_timed_launch tl(c, "khop_init");
            hipLaunchKernelGGL(vgl_k_khop_check, dim3(vgl_grid(n, VGL_BLOCK, SUB_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, d_seeds, n, cnt.p);
        }
        VGL_HIP_TRY(hipGetLastError());
        VGL_TRY(vgl_publish_counters(c, "khop_publish", cnt, KH_NCNT));
        if (c->h_counters[KH_BAD] != 0) VGL_FAIL("khop_run: a seed is outside [0, V)");
    }
    if ((symmetric || direction == 1) && !g->transposed) {            // the handle with the two directions swapped, as scc keeps it
        vgl_hip_graph *t = nullptr;
        VGL_TRY(vgl_hip_graph_create(c, V, 0, V, g->in.rowptr, g->in.adj, g->in.edges, g->out.rowptr, g->out.adj, g->out.edges, &t));
        g->transposed.reset(t);
    }
    {
        vgl_timed_launch tl(c, "khop_init");
        hipLaunchKernelGGL(vgl_k_khop_fill, dim3(vgl_grid(V, VGL_BLOCK, SUB_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, d_hop);
    }
    if (n > 0) {
        vgl_timed_launch tl(c, "khop_init");
        hipLaunchKernelGGL(vgl_k_khop_seed, dim3(vgl_grid(n, VGL_BLOCK, SUB_MAX_GRID)), dim3(VGL_BLOCK), 0, st, d_seeds, n, d_hop);
    }
    VGL_HIP_TRY(hipGetLastError());
    vgl_hip_graph *follow[2] = {nullptr, nullptr};
    int nfollow = 0;
    if (symmetric || direction == 0) follow[nfollow++] = g;
    if (symmetric || direction == 1) follow[nfollow++] = g->transposed.get();
    for (int32_t level = 0; level < hops && n > 0; level++) {
        int64_t F = 0, M = 0;
        for (int k = 0; k < nfollow; k++) {                           // (a vertex the first step reaches holds level + 1: it is no frontier of the second)
            int64_t f = 0, m = 0;
            VGL_TRY(vgl_hip_bfs_step_top_down(c, follow[k], d_hop, level, nullptr, &f, &m));
            F = f;
            M += m;
        }
        if (F == 0) break;
        out.levels_run++;
        out.frontier_total += F;
        out.edges_examined += M;
    }
    {
        vgl_timed_launch tl(c, "khop_count");
        hipLaunchKernelGGL(vgl_k_khop_reached, dim3(vgl_grid(V, VGL_BLOCK, SUB_MAX_GRID)), dim3(VGL_BLOCK), 0, st, V, (const int32_t *)d_hop, cnt.p);
    }
    VGL_HIP_TRY(hipGetLastError());
    VGL_TRY(vgl_publish_counters(c, "khop_publish", cnt, KH_NCNT));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.reached = c->h_counters[KH_REACHED];
    if (stats) *stats = out;
    return 0;
}

int vgl_hip_sample_neighbors(vgl_hip_ctx *c, vgl_hip_graph *g, const int32_t *d_seeds, int64_t n, int32_t fanout, int direction, uint32_t seed, int64_t *d_rowptr,
                             int32_t *d_adj, int64_t *d_origin, vgl_hip_sample_stats *stats)
{
    if (!c || !g) VGL_FAIL("sample_neighbors: null argument");
    if (sub_sharded(g)) VGL_FAIL("sample_neighbors: graph handle must own all rows (sampling has no sharded form)");
    if (n < 0 || n >= ((int64_t)1 << 31)) VGL_FAIL("sample_neighbors: n must be in [0, 2^31)");
    if (n > 0 && !d_seeds) VGL_FAIL("sample_neighbors: d_seeds must not be NULL");
    if (fanout < 1) VGL_FAIL("sample_neighbors: fanout must be at least 1");
    if (direction != 0 && direction != 1) VGL_FAIL("sample_neighbors: direction must be 0 (outgoing) or 1 (incoming)");
    if (direction == 1 && !g->in.rowptr) VGL_FAIL("sample_neighbors: direction 1 needs the incoming CSR");
    if (!d_rowptr || (n > 0 && !d_adj)) VGL_FAIL("sample_neighbors: d_rowptr and d_adj must not be NULL");
    const vgl_dir_csr &csr = direction == 0 ? g->out : g->in;
    if (csr.edges >= ((int64_t)1 << 32)) VGL_FAIL("sample_neighbors: the adjacency array has 2^32 entries or more (the keys of its positions would tie)");
    hipStream_t st = c->stream;
    const vgl_rc_bounds b = vgl_rc_env_bounds(c, "VGL_SAMPLE_SHORT", "VGL_SAMPLE_WAVE");
    vgl_hip_sample_stats out;
    memset(&out, 0, sizeof(out));
    out.seeds = n;
    vgl_dev<unsigned long long> cnt;
    vgl_dev<int64_t> count;
    vgl_scratch tmp;
    vgl_rc_lists<vgl_rc_bounded> L;
    VGL_TRY(vgl_open_counters(c, &cnt, SMP_NCNT));
    VGL_TRY(count.alloc(st, (size_t)n + 1));
    VGL_HIP_TRY(hipMemsetAsync(count.p + n, 0, sizeof(int64_t), st));
    smp_src src{g->V, csr.rowptr, d_seeds, fanout, b, count.p};
    VGL_TRY(L.count(c, "sample_count", "sample_publish", src, n, SUB_MAX_GRID, cnt.p, SMP_NCNT, SMP_ROWS, SMP_BAD, SMP_EXAM, n, "sample_neighbors: a seed is outside [0, V)",
                    "sample_neighbors: internal error (the classes do not add up to the seeds)"));
    const int64_t *rows = L.rows;
    out.rows_short = rows[0]; out.rows_wave = rows[1]; out.rows_wg = rows[2];
    out.entries_examined = c->h_counters[SMP_EXAM];
    // from here on the outputs are written
    VGL_TRY(vgl_exclusive_scan(c, tmp, count.p, d_rowptr, (size_t)n + 1, VGL_SIZE_ONLY));
    {
        vgl_timed_launch tl(c, "sample_count");
        VGL_TRY(vgl_exclusive_scan(c, tmp, count.p, d_rowptr, (size_t)n + 1));
    }
    VGL_HIP_TRY(hipMemcpyAsync(cnt.p + SMP_TOTAL, d_rowptr + n, sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (n > 0) {
        src.count = nullptr;                                          // (the seeds are validated and counted)
        VGL_TRY(L.fill(c, "sample_count", src, n, SUB_MAX_GRID, 1, nullptr, cnt + SMP_TAIL));
        const smp_args a{csr.rowptr, csr.adj, d_seeds, d_rowptr, d_adj, d_origin, fanout, vgl_fmix32(seed + 0x9e3779b9u)};
        const char *const slot[VGL_RC_N] = {"sample_short", "sample_wave", "sample_wg"};
        const int32_t *const list[VGL_RC_N] = {L.l[0].rows, L.l[1].rows, L.l[2].rows};
        VGL_TRY(vgl_rc_launch_trio(c, slot, rows, sub_grid_cap, vgl_k_sample_group<VGL_RC_SHORT>, vgl_k_sample_group<VGL_RC_WAVE>, vgl_k_sample_wg, list, a));
    }
    VGL_TRY(vgl_publish_counters(c, "sample_publish", cnt, SMP_NCNT));
    VGL_HIP_TRY(hipStreamSynchronize(st));
    out.sampled_total = c->h_counters[SMP_TOTAL];
    out.algorithmic_bytes = 60 * n + 16 * (n + 1) + 8 * out.sampled_total;
    if (stats) *stats = out;
    return 0;
}

}  // extern "C"
