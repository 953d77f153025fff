// vgl_hip_internal.h -- shared host/device internals of libvgl_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <map>
#include <memory>
#include <vector>
#include "../../include/vgl_hip.h"

// ---------------------------------------------------------------------------------------------
// geometry: 256-thread workgroups (4 wavefronts of 64), edge tiles of 2048 entries (8 per thread)
// ---------------------------------------------------------------------------------------------
constexpr int VGL_BLOCK = 256;
constexpr int VGL_EPT = 8;
constexpr int VGL_TILE = VGL_BLOCK * VGL_EPT;      // 2048 edges (or vertices) per workgroup tile
constexpr int VGL_WAVES = VGL_BLOCK / 64;
constexpr int VGL_FOLD_WORDS = 2048;     // the folded frontier of the filtered bottom-up probe: 2^17 bits = 16 KiB of LDS per workgroup

int vgl_set_error(const char *file, int line, const char *msg);
#define VGL_FAIL(msg) return vgl_set_error(__FILE__, __LINE__, (msg))
#define VGL_HIP_TRY(expr)                                                          \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) return vgl_set_error(__FILE__, __LINE__, hipGetErrorString(_e)); \
    } while (0)
#define VGL_TRY(expr)            \
    do {                         \
        int _s = (expr);         \
        if (_s != 0) return _s;  \
    } while (0)

// device counters (int64 slots in ctx->d_counters, mirrored into pinned host memory on demand)
enum {
    C_FRONT = 0, C_NEIGH = 1, C_BU_FOUND = 2, C_BU_EDGES = 3, C_HEAVY = 4, C_CHANGED = 5,
    C_EDGES = 6, C_TMP0 = 7, C_TMP1 = 8, C_JUMP = 9,
    C_NEXT_F = 10, C_NEXT_M = 11,    // device only: size / out-degree sum of the frontier an emitting top-down level (or the list kernel) just produced
    C_SKIPPED = 12, C_HINT = 13,     // host mirror only: the bitmap count skipped its degree pass (the level turns bottom-up) / the list kernel left C_NEXT_*
    C_SUM_CHECK = 14,                // device only: VGL_HIP_SUM_* bits of the sum over edges, kept until vgl_hip_sum_over_edges_check takes them
    C_NSLOTS = 32
};
// sharded accumulators: kernels launched with very many workgroups add into shard (blockIdx & (VGL_NSHARD-1)) so that no
// single address receives more than a few hundred device atomics; vgl_read_counters folds them into the counter slots.
constexpr int VGL_NSHARD = 1024;

struct vgl_timing_slot {
    int64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
};

// Tunables of the fused traversal (DESIGN "Run-time switches"), parsed from the environment when the context is created and again only when the
// process environment has changed since (vgl_ctx_refresh_env: one pass over the pointers of `environ`, no string is looked at) -- not a dozen
// getenv() per traversal.  A negative / NaN value = "not set": the traversal derives its default from the graph.
struct vgl_bfs_tunables {
    int64_t td_emit_edges = -1, small_m = -1, bm_expand = -1, shard_td_emit_edges = -1, filter_f = -1;
    double td_filter_share = -1.0, td_late_share = -1.0, blocked_share = -1.0;
    int shard_sparse_cap = -1;
    bool no_hint = false, no_scan_bound = false, trace = false;
    // vgl_hip_bfs_run_batch: 1 = every traversal after the first re-initialises [0, reach_rows) instead of running at a level offset; the offset
    // beyond which a traversal does so anyway (default INT32_MAX - V - 2; the tests lower it)
    bool batch_refill = false;
    int64_t offset_limit = -1;
};

struct vgl_hip_ctx {
    std::map<std::string, std::string> env;      // the VGL_* variables as they stood at the last refresh
    uint64_t env_signature = 0;
    vgl_bfs_tunables bfs;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t *d_counters = nullptr;   // C_NSLOTS
    int64_t *d_shards = nullptr;     // VGL_NSHARD accumulators folded into d_counters[C_EDGES]
    int64_t *h_counters = nullptr;   // pinned mirror (+ publish sequence number at [C_NSLOTS])
    int64_t publish_seq = 0;
    double *d_partials = nullptr;    // reduction partials (f64), capacity partials_cap
    size_t partials_cap = 0;
    bool timing = false;
    std::string timing_only;          // when not empty: only launches under this name are bracketed by events
    int timing_stride = 1;            // ... and of those only every stride-th
    int64_t timing_seen = 0;
    std::map<std::string, vgl_timing_slot> slots;
    std::vector<hipEvent_t> event_pool;
};

// the environment as the context sees it: refresh at the entry of a run (cheap when nothing changed), then read from the snapshot
void vgl_ctx_refresh_env(vgl_hip_ctx *c);
const char *vgl_env(vgl_hip_ctx *c, const char *name);            // refreshes, then looks up; nullptr when unset (use the value at once)
int64_t vgl_env_int(vgl_hip_ctx *c, const char *name, int64_t dflt, int64_t lo, int64_t hi);    // unset or empty: dflt; always within [lo, hi]

// Large, short-lived or plan-sized device buffers come from a stream-ordered memory pool OWNED BY THIS LIBRARY (one per device, created on
// first use: hipMemPoolCreate + hipMallocFromPoolAsync on the context's stream; the device's default pool, which other hipMallocAsync
// users of the process share, is left as it was found).  The pool keeps what is freed up to VGL_POOL_KEEP_GB (default 48 GiB): a plain
// hipMalloc right after tens of GB were hipFree'd was measured to stall for 0.5 - 1.3 s on this driver, and fresh mappings cost ~14 ms
// per GB on first touch; pool memory that has been used once costs neither.  vgl_hip_ctx_trim / vgl_hip_ctx_destroy hand it back.
hipMemPool_t vgl_lib_pool(int device);          // context.hip; nullptr when the pool could not be created (callers fall back to hipMallocAsync)
// LARGE blocks do not come from the pool (round 5, late).  Kernels that touched a freshly grown multi-GB pool block ended in a GPU memory fault in
// 2 - 12 % of the processes that built an RMAT-24 graph (apps/bin/*_hip -s 24: `GPU coredump`, exit by SIGPIPE, the bench's operator leg lost a row;
// profiles/r05_pool_fault_ab.log: 7 of 60 runs with the scratch of vgl_hip_coo_to_csr from the pool, 0 of 60 with it from hipMalloc; ROCm 7.2; the
// round's first workaround drew the line at 2^33 bytes, where the fault was first seen).  Blocks of at least vgl_pool_block_limit() bytes
// (VGL_POOL_MAX_MB, default 64 MiB) are plain hipMalloc blocks, remembered so that vgl_pool_free hands them to hipFree after a stream
// synchronisation; the pool keeps what it is good at, the many small buffers of a plan build.
size_t vgl_pool_block_limit();                  // context.hip
void vgl_big_block_remember(void *p);           // context.hip: p came from hipMalloc
bool vgl_big_block_forget(void *p);             // context.hip: true (and forgotten) when p came from hipMalloc
static inline hipError_t vgl_pool_alloc(hipStream_t st, void **p, size_t bytes)
{
    if (bytes >= vgl_pool_block_limit()) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) vgl_big_block_remember(*p);
        return e;
    }
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess)
        if (hipMemPool_t pool = vgl_lib_pool(dev)) return hipMallocFromPoolAsync(p, bytes ? bytes : 16, pool, st);
    return hipMallocAsync(p, bytes ? bytes : 16, st);
}
static inline void vgl_pool_free(hipStream_t st, void *p)
{
    if (!p) return;
    if (vgl_big_block_forget(p)) { (void)hipStreamSynchronize(st); (void)hipFree(p); }      // (kernels of this stream may still use it)
    else (void)hipFreeAsync(p, st);
}
// One owned device block of T: freed by the destructor, move-only (a copy -- a buffer object handed to a kernel by value -- would be a double
// free, so it does not compile), read as a plain T * everywhere else.  Where the block comes from is chosen where it is allocated and never
// changes: alloc(n) is hipMalloc / hipFree, alloc(st, n) the stream-ordered path above (the buffer remembers the stream).  A struct that owns
// device memory holds it in members of this type; whoever deletes the struct synchronises the stream first (kernels may still use the blocks).
template <class T>
struct vgl_dev {
    T *p = nullptr;
    hipStream_t st = nullptr;
    bool pooled = false;
    vgl_dev() = default;
    vgl_dev(const vgl_dev &) = delete;
    vgl_dev &operator=(const vgl_dev &) = delete;
    vgl_dev(vgl_dev &&o) noexcept : p(o.p), st(o.st), pooled(o.pooled) { o.p = nullptr; }
    vgl_dev &operator=(vgl_dev &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; st = o.st; pooled = o.pooled; o.p = nullptr; }
        return *this;
    }
    ~vgl_dev() { reset(); }
    operator T *() const { return p; }
    int alloc(size_t n)                             // n elements (none: a minimal block), replacing what was held
    {
        reset();
        pooled = false;
        return held(hipMalloc((void **)&p, sizeof(T) * (n ? n : 1)));
    }
    int alloc(hipStream_t stream, size_t n)
    {
        reset();
        pooled = true; st = stream;
        return held(vgl_pool_alloc(stream, (void **)&p, sizeof(T) * (n ? n : 1)));
    }
    int held(hipError_t e)
    {
        if (e != hipSuccess) p = nullptr;
        VGL_HIP_TRY(e);
        return 0;
    }
    void reset()
    {
        if (!p) return;
        if (pooled) vgl_pool_free(st, p); else (void)hipFree(p);
        p = nullptr;
    }
};

struct vgl_dir_csr {                 // one direction of the graph (borrowed) + derived tile table (owned)
    const int64_t *rowptr = nullptr; // nrows+1, rebased to 0
    const int32_t *adj = nullptr;    // global vertex ids
    int64_t edges = 0;
    vgl_dev<int32_t> tile_row;       // ntiles+1: local row that contains edge t*VGL_TILE
    int64_t ntiles = 0;
    vgl_dev<int32_t> hub_rows;     // pull sums (PageRank, HITS): rows with >= 512 edges grouped per wavefront + offsets (lazy)
    int32_t nhubs = 0;
    int hub_blocks = 0;              // workgroups of the pull kernel that run the hub schedule
    vgl_dev<int32_t> giant_rows;   // rows of at least VGL_PULL_GIANT_DEGREE entries, grouped per workgroup + offsets (the workgroup scheme of vgl_pull.h)
    int ngiants = 0, giant_blocks = 0;
    vgl_dev<int32_t> hub_chunks;   // unordered hub sums (HITS): per chunk (row, first entry - row start in units of VGL_PULL_CHUNK); then, per hub in
                                     // row order, (row, first chunk, chunks) triples -- see vgl_pull_find_hubs
    int n_hub_chunks = 0, n_hub_list = 0;
    vgl_dev<double> hub_chunk_sums;
    vgl_dev<int32_t> pull_blk_row; // pull sums: first row of every ordinary workgroup (+ end): <= 256 rows and ~16 K edges each (lazy)
    int pull_nblk = 0;
    int64_t max_row = -1;            // longest row (lazy; PageRank's choice between the ordered and the blocked pull)
};

// The lazy per-algorithm caches of a graph handle.  Their types are complete in their own files only, so the handle deletes them through a function
// that the owner's file defines for its type (template <> void vgl_cache_free(vgl_x_cache *p) { delete p; }).
template <class T> void vgl_cache_free(T *p);
template <class T> struct vgl_cache_delete { void operator()(T *p) const { vgl_cache_free(p); } };
template <class T> using vgl_cache = std::unique_ptr<T, vgl_cache_delete<T>>;
struct vgl_hip_graph {
    uint64_t uid = 0;                // unique per created handle (a freed handle's address may be reused: caches key on this, not on the pointer)
    int32_t V = 0, row_begin = 0, row_end = 0, nrows = 0;
    vgl_dir_csr out, in;
    // scratch shared by the fused algorithms (allocated at creation, sized by V / nrows / edges)
    vgl_dev<uint64_t> bm_visited, bm_front, bm_next; // ceil(V/64)+1 words each
    vgl_dev<uint64_t> bm_fold;     // VGL_FOLD_WORDS words: bm_front folded onto 2^17 bits for the filtered bottom-up probe (vgl_k_front_fold, bfs.hip)
    vgl_dev<uint64_t> bm_in_nz;    // bit v = owned vertex v has incoming edges (bottom-up candidates)
    vgl_dev<int32_t> in_head;      // two planes of 16-byte records (in-neighbours 0-3 and 4-7 of the eight smallest ids, -1 padded), ONE RECORD PER
                                     // OWNED ROW THAT HAS INCOMING EDGES, in row order: record index = in_nz_rank[group] + rank of the row among the set
                                     // bits of its in_nz word -- the rows without incoming edges (45 % of an RMAT graph) are never bottom-up
                                     // candidates and used to take half of every 128-byte line of the planes
    bool in_head_packed = false;     // the records are 12 bytes (four 24-bit ids, 0xFFFFFF = absent; two planes of in_nz_rows x 12 bytes): chosen once, when
                                     // the records are built, iff every id in them is below 0xFFFFFF (VGL_BFS_HEADS; graph_frontier.hip)
    vgl_dev<int32_t> in_nz_rank;   // per 64-row group: number of owned rows with incoming edges before the group
    int32_t in_nz_rows = 0;          // owned rows with incoming edges = records per plane
    int32_t reach_rows = 0;          // 1 + the largest owned vertex with an incoming edge (0: none has one; V when the incoming CSR is not stored): a
                                     // traversal writes levels[v] only for v below it and for its own source, so the fused BFS scans and re-initialises
                                     // [0, reach_rows) only.  Read off the graph (bm_in_nz), not off the numbering: close to V unless the rows without
                                     // incoming edges are numbered last (a degree-sorted RMAT graph: 38 % of the rows)
    vgl_dev<int32_t> pr_indeg;     // sharded PageRank: in-degrees minus self loops of ALL vertices, summed over the ranks once per graph handle
    bool pr_indeg_ready = false;
    vgl_dev<uint64_t> bm_in_long;  // bit v = owned vertex v has more than 8 incoming edges (deferred to the wavefront pass when it misses)
    vgl_dev<int32_t> ids;          // nrows
    vgl_dev<int64_t> offs;         // nrows+1
    vgl_dev<int32_t> vt_cnt, vt_cnt_off;   // per vertex tile
    vgl_dev<int64_t> vt_deg, vt_deg_off;
    int64_t nvtiles = 0;
    vgl_dev<int32_t> vt_min_deg;   // per vertex tile: smallest out-degree of its rows (lower bound of a frontier's edge count from its per-tile sizes)
    vgl_dev<uint8_t> gnf_bits;     // generate_new_frontier of the operator classes: the predicate's bits (byte v >> 3, bit v & 7; lazy, V / 8 bytes) -- the
                                     // compaction of a SPARSE result reads these 2 MiB instead of 64 MiB of int32 flags (vgl_hip_gnf_begin / _complete)
    vgl_dev<int32_t> tile_first;   // out.ntiles + 2
    vgl_dev<int32_t> heavy;        // nrows + slack: per-workgroup segments of deferred bottom-up vertices
    vgl_dev<int64_t> bu_partials;  // 4 partial counters per bottom-up workgroup
    vgl_dev<uint32_t> tickets;     // arrival counters of the "last workgroup finishes the job" kernels (reset by that workgroup)
    vgl_dev<int32_t> epoch;        // V (SSSP active filter)
    vgl_dev<float> fscratch;       // V (PR contrib)
    vgl_dev<float> fscratch2;      // V (PR rdeg)
    vgl_dev<float> fscratch3;      // V (PR new ranks)
    vgl_dev<int32_t> iscratch;     // V (PR indeg when not supplied)
    std::unique_ptr<vgl_hip_graph> transposed;   // SCC: handle with the two directions swapped (backward reach = BFS on it), lazy, owned
    // blocked layouts (vgl_blocked.h): lazy, shared with the plans built over them -- the graph drops its reference, the last holder frees
    std::shared_ptr<const struct vgl_blocked_layout> blk_pr;    // PageRank's blocked pull over the outgoing CSR
    std::shared_ptr<const struct vgl_blocked_layout> blk_cc;    // the Shiloach-Vishkin hook as a blocked pass
    std::shared_ptr<const struct vgl_blocked_layout> blk_bfs;   // the large top-down BFS levels as a blocked pass (vgl_hip_bfs_prepare_blocked)
    std::shared_ptr<const struct vgl_blocked_layout> blk_path;  // the path layouts (Bellman-Ford / widest-path pull: rows gather, edge index kept): built
                                                                // once per graph, every vgl_hip_sssp_pull_plan is a plan over it with weights of its own
    std::string blk_path_key;                    // the layout switches it was built under (fuse threshold, unit sizes, piece bound: the tests vary them per plan)
    vgl_cache<struct vgl_lp_cache> lp[2];        // label propagation: degree classes, hub and push schedules of the out / in CSR (lp.hip, lazy, owned)
    vgl_cache<struct vgl_tri_cache> tri;         // triangle counting: the oriented CSR, undirected degrees and row classes (tri.hip, lazy, owned)
    vgl_cache<struct vgl_bc_cache> bc;           // betweenness centrality: the row classes of both directions (bc.hip, lazy, owned)
    vgl_cache<struct vgl_msbfs_cache> msbfs;     // multi-source BFS: the row classes and the rows by class of both directions (msbfs.hip, lazy, owned)
    vgl_cache<struct vgl_simple_cache> simple;   // k-core, k-truss, minimum spanning forest, biconnectivity: the symmetric simple CSR, its edge ids and the edge id of
                                                 // every stored entry, in three lazy stages (vgl_simple.h, simple.hip; owned)
    vgl_cache<struct vgl_sim_cache> sim;         // vertex similarity: the 2-paths that leave every vertex (sim.hip, lazy, owned)
    vgl_cache<struct vgl_ppr_cache> ppr;         // personalised PageRank: the sorted row-class lists and the chunks of the pull directions (ppr.hip, lazy, owned)
};

struct vgl_hip_frontier {
    vgl_hip_graph *g = nullptr;
    int32_t *flags = nullptr;        // V: what the kernels use -- own_flags / own_ids below, or the arrays of the caller of vgl_hip_frontier_create_on
    int32_t *ids = nullptr;          // V
    vgl_dev<int32_t> own_flags, own_ids;   // empty when the frontier borrows its arrays
    int32_t size = 0;
    int64_t neighbours = 0;
    int sparsity = VGL_HIP_FRONTIER_ALL_ACTIVE;
    // advance plan of a SPARSE frontier (built on demand by vgl_hip_frontier_advance_plan)
    vgl_dev<int64_t> offs;           // V+1 exclusive edge offsets of ids[] in the planned direction
    vgl_dev<int32_t> tile_first;     // ceil(E/VGL_TILE)+2
    vgl_dev<int64_t> blk_sum, blk_off;  // per 2048-id block degree sums / offsets
    int plan_dir = -1;               // direction whose edge offsets `offs` AND tile table `tile_first` describe the current ids (-1: none; set by
                                     // vgl_hip_gnf_complete and vgl_hip_frontier_advance_plan, voided by every change of the ids)
    int64_t plan_edges = 0;          // edges of the ids in that direction
};

// a handle while its entry point builds it: an early return deletes it the way its destroy function does, after a stream synchronise
template <class T>
struct vgl_synced_delete {
    vgl_hip_ctx *c;
    void operator()(T *p) const { (void)hipStreamSynchronize(c->stream); delete p; }
};
template <class T> using vgl_building = std::unique_ptr<T, vgl_synced_delete<T>>;

// timing helpers (no-ops unless ctx->timing)
struct vgl_timed_launch {
    vgl_hip_ctx *ctx; vgl_timing_slot *slot; hipEvent_t a, b;
    vgl_timed_launch(vgl_hip_ctx *c, const char *name);
    ~vgl_timed_launch();
};

int vgl_read_counters(vgl_hip_ctx *ctx, bool fold_shards = true);   // D2H all slots into h_counters, synchronises
// kernels that publish their own results (last workgroup writes the slots it produced + `seq` into the pinned mirror):
// seq = vgl_next_seq() is passed to the kernel, vgl_wait_counters(seq) spins until it shows up
int64_t vgl_next_seq(vgl_hip_ctx *ctx);
int vgl_wait_counters(vgl_hip_ctx *ctx, int64_t seq);
// counters of an algorithm's own (n <= C_NSLOTS): cnt[0 .. n) into h_counters by one launch under the timing slot `slot`, then waits for them
int vgl_publish_counters(vgl_hip_ctx *ctx, const char *slot, const unsigned long long *cnt, int n);
int vgl_zero_counters(vgl_hip_ctx *ctx, int first, int count);
// the n device counters of a call, all 0
static inline int vgl_open_counters(vgl_hip_ctx *ctx, vgl_dev<unsigned long long> *cnt, int n)
{
    VGL_TRY(cnt->alloc(ctx->stream, (size_t)n));
    VGL_HIP_TRY(hipMemsetAsync(cnt->p, 0, sizeof(unsigned long long) * (size_t)n, ctx->stream));
    return 0;
}
// the murmur3 finaliser: a bijection of uint32
__host__ __device__ inline uint32_t vgl_fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
int vgl_ensure_partials(vgl_hip_ctx *ctx, size_t n);
int vgl_build_tile_rows(vgl_hip_ctx *ctx, struct vgl_dir_csr &d, int32_t nrows);     // d.tile_row / d.ntiles from d.rowptr / d.edges (owned by the caller)
// The direction rule itself (gpu_change_state, change_state.hpp:100-141), for the host loops and the count launch alike: the same exact int64_t
// arithmetic on both sides, so that they reach the same decision.  `visited` counts the vertices visited so far WITH the frontier F about to be
// expanded; M is its out-degree sum.
constexpr int VGL_DO_ALPHA = 15;       // change_state.hpp:5
constexpr int VGL_DO_BETA = 18;        // change_state.hpp:6
__host__ __device__ inline int64_t vgl_do_factor(int64_t E, int64_t V) { return E / V / 2 > 1 ? E / V / 2 : 1; }     // change_state.hpp:104
// the fewest frontier edges that turn a level bottom-up (at least V / ALPHA, when every vertex is visited)
__host__ __device__ inline int64_t vgl_do_bottom_up_edges(int64_t V, int64_t visited, int64_t factor) { return ((V - visited) * factor + V) / VGL_DO_ALPHA; }
__host__ __device__ inline bool vgl_do_turn_bottom_up(int64_t F, int64_t M, int64_t prev_f, int64_t visited, int64_t V, int64_t factor)
{
    return F > prev_f && M >= vgl_do_bottom_up_edges(V, visited, factor);
}
// back to top-down in the "shrinking phase" = not growing (change_state.hpp:106,121)
__host__ __device__ inline bool vgl_do_turn_top_down(int64_t F, int64_t prev_f, int64_t visited, int64_t V, int64_t factor)
{
    return F <= prev_f && F < ((V - visited) * factor + V) / (factor * VGL_DO_BETA);
}
// frontier from a bitmap over the owned words (bfs.hip): count = sizes to h_counters[C_FRONT / C_NEIGH] (waits), write = ids + edge offsets + tile table
// what the direction rule (gpu_change_state) needs besides the new frontier's F and M: with it the count launch may find on the device that
// the level turns bottom-up and leave out everything a top-down level would need (degree sums, compaction offsets)
struct vgl_do_hint { int64_t prev_f, visited_total, V, factor; };
int vgl_bfs_bm_gnf(vgl_hip_ctx *c, struct vgl_hip_graph *g, const uint64_t *front, bool count, bool write, int64_t M_known = -1, bool advance = false,
                   const vgl_do_hint *hint = nullptr);
// set bits of `words` 64-bit words as ids (64 * (word_base + word) + bit): d_out[0] = their number, d_out[1 .. 1 + cap) = the first cap handed out
int vgl_bitmap_to_ids(vgl_hip_ctx *c, int64_t words, const uint64_t *d_bits, int64_t word_base, int32_t cap, int32_t *d_out);
int vgl_zero_words(vgl_hip_ctx *c, uint64_t *d_words, int64_t words);      // one launch (bfs.hip)

static inline int64_t vgl_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// workgroups of a grid-stride launch: one per `per_block` units of work, at least 1, at most cap
static inline unsigned vgl_grid(int64_t work, int64_t per_block, int64_t cap)
{
    const int64_t n = vgl_ceil_div(work, per_block);
    return (unsigned)(n < 1 ? 1 : n > cap ? cap : n);
}

// ---------------------------------------------------------------------------------------------
// device helpers (wave = 64 lanes)
// ---------------------------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ int vgl_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ int vgl_wave() { return threadIdx.x >> 6; }

// true in exactly one workgroup per launch: the last one to get here.  Protocol (cheap on a multi-XCD part: a device-scope
// release FENCE writes back the whole L2 of the XCD -- every workgroup doing that made a BFS 2.4x slower):
//   * what the last workgroup must see is written by THREAD 0 with vgl_put_agent (device-scope atomic exchange) BEFORE the
//     call, and the values the exchanges RETURN are folded into `dep`: the ticket increment is made data-dependent on them, so
//     it cannot be issued before the exchanges have completed at the coherence point (no fence, no cache write-back);
//   * the last workgroup reads those values with vgl_load_agent (device-scope atomic load).
// Call from all threads of every workgroup (dep only matters in thread 0); the ticket is left at 0 for the next launch.
__device__ __forceinline__ uint32_t vgl_put_agent(int32_t *p, int32_t v) { return (uint32_t)atomicExch(p, v); }
__device__ __forceinline__ uint32_t vgl_put_agent(int64_t *p, int64_t v)
{
    return (uint32_t)atomicExch(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}
template <class T> __device__ __forceinline__ void vgl_store_agent(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> __device__ __forceinline__ T vgl_load_agent(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// Tickets are two-level: same-address device atomics serialise (~12 ns each: 2048 workgroups on one counter cost 25 us, more than
// the launches this saves), so workgroup b arrives at sub-counter b % 32 (its own cache line) and only the last arrival of a
// sub-counter moves on to the top counter: ~64 + 32 serialised atomics instead of 2048.
constexpr int VGL_TICKET_FAN = 32;
constexpr int VGL_TICKET_STRIDE = 16;                                  // uint32 per counter: one 64-byte line each
constexpr int VGL_TICKET_WORDS = (VGL_TICKET_FAN + 1) * VGL_TICKET_STRIDE;
__device__ __forceinline__ bool vgl_last_block(uint32_t *ticket, uint32_t dep)
{
    __shared__ int s_is_last;
    if (threadIdx.x == 0) {
        uint32_t one = 1u;
        asm volatile("" : "+v"(one) : "v"(dep));                     // `one` now depends on the returned values
        const uint32_t nb = gridDim.x, sub = blockIdx.x % VGL_TICKET_FAN;
        const uint32_t expect = (nb - sub + VGL_TICKET_FAN - 1) / VGL_TICKET_FAN;           // workgroups with this residue
        uint32_t *sub_ticket = ticket + (1 + sub) * VGL_TICKET_STRIDE;
        bool last = false;
        if (__hip_atomic_fetch_add(sub_ticket, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == expect - 1) {
            vgl_store_agent(sub_ticket, 0u);
            const uint32_t groups = nb < (uint32_t)VGL_TICKET_FAN ? nb : (uint32_t)VGL_TICKET_FAN;
            if (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1) {
                vgl_store_agent(ticket, 0u);
                last = true;
            }
        }
        s_is_last = last;
    }
    __syncthreads();
    return s_is_last != 0;
}
// results of a last workgroup go to the device counters and straight into the pinned host mirror, then the sequence number
__device__ __forceinline__ void vgl_publish2(int64_t *counters, volatile int64_t *host, int64_t seq, int slot_a, int64_t a, int slot_b, int64_t b)
{
    counters[slot_a] = a; counters[slot_b] = b;
    host[slot_a] = a; host[slot_b] = b;
    __threadfence_system();
    host[C_NSLOTS] = seq;
    __threadfence_system();
}

template <class T>
__device__ __forceinline__ T vgl_wave_incl_add(T v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        T n = __shfl_up(v, o);
        if (vgl_lane() >= o) v += n;
    }
    return v;
}
__device__ __forceinline__ int vgl_wave_incl_max(int v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int n = __shfl_up(v, o);
        if (vgl_lane() >= o) v = max(v, n);
    }
    return v;
}
template <class T>
__device__ __forceinline__ T vgl_wave_reduce_add(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ void vgl_atomic_add64(int64_t *p, int64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }
// every lane of the wave, once, at the end of a kernel: the wave's sum of m goes to *slot by one atomic (none when it is 0)
__device__ __forceinline__ void vgl_wave_flush_add(unsigned long long *slot, int64_t m)
{
    m = vgl_wave_reduce_add(m);
    if (vgl_lane() == 0 && m) atomicAdd(slot, (unsigned long long)m);
}
// Every lane of the wave calls (uniform control flow).  The lanes with `want` append id to lists[cls] (NCLS lists of `cap` entries each): one returning
// atomic per wave and class.  tail: the NCLS cumulative list lengths, in global memory or in LDS.
template <int NCLS>
__device__ __forceinline__ void vgl_wave_append(bool want, int32_t id, int cls, int32_t *const *lists, int32_t cap, unsigned long long *tail)
{
    if (!__any(want)) return;
    const int lane = vgl_lane();
#pragma unroll
    for (int c = 0; c < NCLS; c++) {
        const bool mine = want && cls == c;
        const unsigned long long m = __ballot(mine);
        if (!m) continue;                                             // (uniform)
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(tail + c, (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
        if (mine) {
            const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (pos < (unsigned long long)cap) vgl_store_agent(lists[c] + pos, id);
        }
    }
}
// the row u of a CSR with rp[u] <= e < rp[u + 1] (0 <= e < rp[V])
__device__ __forceinline__ int32_t vgl_row_of(const int64_t *rp, int32_t V, int64_t e)
{
    int32_t lo = 0, hi = V;                     // invariant: rp[lo] <= e < rp[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (rp[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}
// the slot of `w` in the ascending entries [lo, hi) of adj, or -1
__device__ __forceinline__ int64_t vgl_slot_of(const int32_t *adj, int64_t lo, int64_t hi, int32_t w)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const int32_t x = adj[mid];
        if (x < w) lo = mid + 1; else if (x > w) hi = mid; else return mid;
    }
    return -1;
}
// x in adj[s, s + n) (ascending, no duplicates)?
__device__ __forceinline__ bool vgl_contains(const int32_t *adj, int64_t s, int n, int32_t x)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (adj[s + mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && adj[s + lo] == x;
}
// the multiplicative hash of a vertex id into a table of 2^bits slots
__device__ __forceinline__ uint32_t vgl_hash(int32_t x, int bits) { return ((uint32_t)x * 0x9E3779B1u) >> (32 - bits); }

// exclusive block scan (add); smem must hold VGL_WAVES elements of T; returns exclusive prefix, *total = block sum
template <class T>
__device__ __forceinline__ T vgl_block_excl_add(T v, T *smem, T *total)
{
    T inc = vgl_wave_incl_add(v);
    __syncthreads();                       // protect smem reuse across calls
    if (vgl_lane() == 63) smem[vgl_wave()] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < VGL_WAVES; w++) {
        T s = smem[w];
        if (w < vgl_wave()) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}
// exclusive block scan (max) for non-negative ints, identity 0
__device__ __forceinline__ int vgl_block_excl_max(int v, int *smem)
{
    int inc = vgl_wave_incl_max(v);
    __syncthreads();
    if (vgl_lane() == 63) smem[vgl_wave()] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < VGL_WAVES; w++)
        if (w < vgl_wave()) base = max(base, smem[w]);
    int up = __shfl_up(inc, 1);
    if (vgl_lane() == 0) up = 0;
    return max(base, up);
}
template <class T>
__device__ __forceinline__ T vgl_block_reduce_add(T v, T *smem)
{
    v = vgl_wave_reduce_add(v);
    __syncthreads();
    if (vgl_lane() == 0) smem[vgl_wave()] = v;
    __syncthreads();
    T tot = 0;
#pragma unroll
    for (int w = 0; w < VGL_WAVES; w++) tot += smem[w];
    return tot;
}

// Row map of an edge tile.  Positions [0, n) of the tile belong to consecutive "rows" (CSR rows or frontier
// positions) r_first..r_last whose start offsets are starts[r] (int64, monotone).  On return s_map[i] holds
// (row of slot i) - r_first.  Empty rows are skipped naturally (the last row starting at a slot owns it).
// s_map: VGL_TILE ints of LDS; s_w: VGL_WAVES ints.  All threads of the workgroup must call.
__device__ __forceinline__ void vgl_tile_row_map(int *s_map, int *s_w, const int64_t *starts, int64_t e0,
                                                 int r_first, int r_last)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < VGL_EPT; j++) s_map[tid + j * VGL_BLOCK] = 0;
    __syncthreads();
    for (int r = r_first + 1 + tid; r <= r_last; r += VGL_BLOCK) {
        const int64_t q = starts[r] - e0;          // > 0 because r_first contains e0
        if (q < VGL_TILE) atomicMax(&s_map[(int)q], r - r_first);
    }
    __syncthreads();
    int m[VGL_EPT];
    int run = 0;
#pragma unroll
    for (int j = 0; j < VGL_EPT; j++) { run = max(run, s_map[tid * VGL_EPT + j]); m[j] = run; }
    const int pre = vgl_block_excl_max(run, s_w);
#pragma unroll
    for (int j = 0; j < VGL_EPT; j++) s_map[tid * VGL_EPT + j] = max(m[j], pre);
    __syncthreads();
}
#endif  // __HIPCC__
