/*
 * vgl_hip.h -- C ABI of libvgl_hip.so, the MI355X (gfx950) backend for VectorGraphLibrary's
 * frontier-driven advance / compute / reduce / generate_new_frontier hot path.
 *
 * Boundary: the reference selects a backend at compile time as a C++ template class
 * (architecture_independent_api.h:33-43; member list vgl_compute_api/template/
 * graph_abstractions_template.h:44-104; recipe manuals/add_new_architecture.txt:1-7).
 * This C ABI is the layer that class binds to (see INTEGRATION.md and
 * vectorgraphlibrary_amd/hip/vgl_hip.hpp): plain pointers and sizes, opaque
 * handles, `int` status (0 = ok) + vgl_hip_last_error().  All device pointers are raw HIP
 * device pointers owned by the caller unless stated; every call is ordered on the context's
 * stream and returns after the work is ENQUEUED unless it has a host-visible result, in which
 * case it synchronises the stream (the reference GPU backend is synchronous per primitive:
 * vgl_compute_api/gpu/advance_csr.hpp:204).
 *
 * Vertex ids are int32, edge offsets int64, properties 4-byte.
 */
#ifndef VGL_HIP_H
#define VGL_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VGL_HIP_ABI_VERSION 1

typedef struct vgl_hip_ctx vgl_hip_ctx;
typedef struct vgl_hip_graph vgl_hip_graph;
typedef struct vgl_hip_frontier vgl_hip_frontier;

/* ---- context / errors (replaces VGL_RUNTIME::init_library cudaSetDevice path, vgl_runtime.hpp:5-25,
 *      and the throw "literal" convention, apps/bfs/bfs.cpp:53-61) ---- */
int vgl_hip_abi_version(void);
const char *vgl_hip_last_error(void);
/* stream: a hipStream_t created by the caller (e.g. torch's current stream); NULL = the device's default stream */
int vgl_hip_ctx_create(int device, void *stream, vgl_hip_ctx **out);
int vgl_hip_ctx_destroy(vgl_hip_ctx *ctx);
int vgl_hip_ctx_sync(vgl_hip_ctx *ctx);
/* plan builders take their scratch and plan arrays from the device's stream-ordered memory pool, which keeps freed memory cached (a
 * second build of the same size then pays no allocator or first-touch cost); this hands the cached memory back to the driver */
int vgl_hip_ctx_trim(vgl_hip_ctx *ctx);
void *vgl_hip_ctx_stream(vgl_hip_ctx *ctx);

/* ---- device memory (replaces MemoryAPI::allocate_array / move_array_to_device, memory_API.hpp:4-15,100-110) ---- */
int vgl_hip_malloc(vgl_hip_ctx *ctx, size_t bytes, void **dptr);
int vgl_hip_free(vgl_hip_ctx *ctx, void *dptr);
int vgl_hip_memcpy_h2d(vgl_hip_ctx *ctx, void *dst, const void *src, size_t bytes);
int vgl_hip_memcpy_d2h(vgl_hip_ctx *ctx, void *dst, const void *src, size_t bytes);
int vgl_hip_memset(vgl_hip_ctx *ctx, void *dst, int byte_value, size_t bytes);

/* ---- synthetic inputs on the device (GraphGenerationAPI::R_MAT / random_uniform,
 *      graph_generation.hpp:5-51,94-187; weights common_generator.hpp:23-36).  Counter-based, so
 *      any [first_edge, first_edge+count) slice can be produced independently on any rank. ---- */
int vgl_hip_gen_rmat(vgl_hip_ctx *ctx, int scale, int64_t first_edge, int64_t count, uint64_t seed,
                     int a, int b, int c, int d, int relabel, int32_t *d_src, int32_t *d_dst);
int vgl_hip_gen_uniform(vgl_hip_ctx *ctx, int scale, int64_t first_edge, int64_t count, uint64_t seed,
                        int32_t *d_src, int32_t *d_dst);
int vgl_hip_gen_weights(vgl_hip_ctx *ctx, int64_t first_edge, int64_t count, uint64_t seed, float *d_w);

/* ---- COO -> CSR on the device, stable in input order (CSRGraph::import, csr/import.hpp:3-68).
 *      Only edges with row_begin <= src < row_end are kept (edge-cut shard, vect_csr/get_api.hpp:66-94);
 *      d_rowptr has (row_end-row_begin+1) entries rebased to 0, d_adj / d_perm have capacity `count`.
 *      d_perm (optional) receives the INPUT edge index of every CSR position (edges_reorder_indexes).
 *      *kept_out = number of edges kept.  Synchronises. ---- */
int vgl_hip_coo_to_csr(vgl_hip_ctx *ctx, int32_t V, int64_t count, const int32_t *d_src, const int32_t *d_dst,
                       int32_t row_begin, int32_t row_end,
                       int64_t *d_rowptr, int32_t *d_adj, int64_t *d_perm, int64_t *kept_out);
/* out[i] = in[perm[i]] for 4-byte elements (EdgesArray weights follow the CSR order,
 * csr_edges_array.hpp:31-40) */
int vgl_hip_gather_u32(vgl_hip_ctx *ctx, int64_t n, const int64_t *d_perm, const void *d_in, void *d_out);
/* VectCSR-style vertex renumbering (VectorCSRGraph::import, vect_csr/import.hpp:61-99): sorted position =
 * (degree descending, original id ascending).  degree_kind 0 = out-degree, 1 = in-degree, 2 = in+out.  The reference
 * renumbers each direction separately; this backend keeps ONE numbering for both directions so that top-down and
 * bottom-up steps share vertex arrays.  d_fwd[orig] = sorted id, d_bwd[sorted] = orig id (forward/backward_conversion).
 * Hot (high-degree) vertices become contiguous, so the per-edge 4-byte gathers of dist/levels/labels/contrib[dst]
 * mostly hit the XCD L2 instead of costing a fabric line each.  Synchronises. */
int vgl_hip_degree_order(vgl_hip_ctx *ctx, int32_t V, int64_t count, const int32_t *d_src, const int32_t *d_dst,
                         int degree_kind, int32_t *d_fwd, int32_t *d_bwd);
/* the two halves of vgl_hip_degree_order for inputs that are produced in chunks (scale-27 shards): accumulate degrees of a
 * chunk into d_degree (uint32[V], zeroed by the caller), then derive the order from the finished histogram. */
int vgl_hip_degree_hist_add(vgl_hip_ctx *ctx, int64_t count, const int32_t *d_src, const int32_t *d_dst, int degree_kind,
                            uint32_t *d_degree);
int vgl_hip_degree_order_from_degrees(vgl_hip_ctx *ctx, int32_t V, const uint32_t *d_degree, int32_t *d_fwd, int32_t *d_bwd);
/* out[i] = map[in[i]] (relabel ids) and out[i] = in[idx[i]] (permute a vertex array) for 4-byte elements */
int vgl_hip_relabel_i32(vgl_hip_ctx *ctx, int64_t n, const int32_t *d_map, const int32_t *d_in, int32_t *d_out);
int vgl_hip_permute_u32(vgl_hip_ctx *ctx, int64_t n, const int32_t *d_idx, const void *d_in, void *d_out);
/* CC labels computed on a renumbered graph -> labels in ORIGINAL ids: out[orig v] = min original id of v's component.
 * d_comp: labels in sorted numbering (int32[V]); d_scratch: int32[V]. */
int vgl_hip_cc_labels_to_original(vgl_hip_ctx *ctx, int32_t V, const int32_t *d_comp, const int32_t *d_fwd,
                                  const int32_t *d_bwd, int32_t *d_scratch, int32_t *d_out);

/* edge-balanced contiguous vertex ranges (VectorCSRGraph::get_mpi_thresholds, vect_csr/get_api.hpp:66-94):
 * bounds[p] .. bounds[p+1] own ~E/parts edges each.  Host array of parts+1 entries.  Synchronises. */
int vgl_hip_partition_rows(vgl_hip_ctx *ctx, int32_t V, const int64_t *d_rowptr, int parts, int32_t *bounds_host);

/* ---- graph handle: borrows the caller's device CSR (CSRGraph, csr/csr_graph.h:22-87; VGL_Graph holds an
 *      outgoing and an incoming container, vgl_graph.h:7-79).  Rows [row_begin,row_end) are present in each
 *      direction (whole graph: 0..V).  The incoming direction may be NULL when only push algorithms run.
 *      Creation builds the per-tile row tables the edge-balanced kernels use (derived data, owned). ---- */
int vgl_hip_graph_create(vgl_hip_ctx *ctx, int32_t V, int32_t row_begin, int32_t row_end,
                         const int64_t *d_out_rowptr, const int32_t *d_out_adj, int64_t out_edges,
                         const int64_t *d_in_rowptr, const int32_t *d_in_adj, int64_t in_edges,
                         vgl_hip_graph **out);
int vgl_hip_graph_destroy(vgl_hip_ctx *ctx, vgl_hip_graph *g);
/* what creation derived for the bottom-up BFS: owned rows with incoming edges (one head record each per plane), and whether the head
 * records are held in the 12-byte form (four 24-bit ids) instead of 16-byte int4 records (VGL_BFS_HEADS=auto|wide|packed at creation;
 * packed only when every id in a record is below 0xFFFFFF).  reach_rows: 1 + the largest owned vertex that has an incoming edge (0 when none
 * has one, V when the incoming CSR is not stored) -- the fused BFS scans and re-initialises only the levels below it.  Any pointer may be NULL. */
int vgl_hip_graph_info(vgl_hip_graph *g, int32_t *in_nz_rows, int *heads_packed, int32_t *reach_rows);

/* ---- frontier (BaseFrontier, base_frontier.h:5-62; sparsity enum framework_types.h:156-160) ---- */
#define VGL_HIP_FRONTIER_DENSE 0
#define VGL_HIP_FRONTIER_SPARSE 1
#define VGL_HIP_FRONTIER_ALL_ACTIVE 2
int vgl_hip_frontier_create(vgl_hip_ctx *ctx, vgl_hip_graph *g, vgl_hip_frontier **out);
int vgl_hip_frontier_destroy(vgl_hip_ctx *ctx, vgl_hip_frontier *f);
/* a handle over flags / ids arrays the caller owns (device-accessible int32[V] each) -- for a backend bound to the reference's own frontier
 * containers (FrontierCSR / FrontierVectorCSR, base_frontier.h:5-62), whose host code reads and writes those arrays; set_state tells the handle
 * what they hold (size, sum of degrees, sparsity as VGL_HIP_FRONTIER_*) and which graph handle (direction container) the frontier refers to. */
int vgl_hip_frontier_create_on(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_flags, int32_t *d_ids, vgl_hip_frontier **out);
int vgl_hip_frontier_set_state(vgl_hip_ctx *ctx, vgl_hip_frontier *f, vgl_hip_graph *g, int32_t size, int64_t neighbours, int sparsity);
int vgl_hip_frontier_set_all_active(vgl_hip_ctx *ctx, vgl_hip_frontier *f);      /* frontier/.../modification.hpp set_all_active */
int vgl_hip_frontier_clear(vgl_hip_ctx *ctx, vgl_hip_frontier *f);
int vgl_hip_frontier_add_vertex(vgl_hip_ctx *ctx, vgl_hip_frontier *f, int32_t v); /* only into an empty frontier (modification.hpp:33-36) */
int vgl_hip_frontier_info(vgl_hip_ctx *ctx, vgl_hip_frontier *f, int32_t *size, int64_t *neighbours, int *sparsity);
int32_t *vgl_hip_frontier_ids(vgl_hip_frontier *f);    /* device, ascending ids, `size` valid entries when SPARSE */
int32_t *vgl_hip_frontier_flags(vgl_hip_frontier *f);  /* device, int32[V] 0/1 */
/* generate_new_frontier from a caller-filled flags array (generate_new_frontier_worker(CSRGraph&),
 * multicore/generate_new_frontier.hpp:113-164 + copy_if_indexes, copy_if.hpp:128-191): counts, Σdegree,
 * ALL_ACTIVE when size == V else SPARSE with ascending-id compaction.  d_flags may alias the frontier's own flags.
 * dense_threshold > 0 selects the VectCSR rule (size > threshold*V => DENSE, flags only; generate_new_frontier.hpp:67-91). */
int vgl_hip_gnf_from_flags(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_flags, double dense_threshold,
                           vgl_hip_frontier *f);
/* same with the predicate (d_values[v] == value) evaluated in-kernel (BFS on_next_level, bfs.hpp:40-45) */
int vgl_hip_gnf_equal_i32(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_values, int32_t value,
                          double dense_threshold, vgl_hip_frontier *f);

/* ---- plans for the templated advance kernels of the C++ operator class (vectorgraphlibrary_amd/hip/): the edge-balanced
 *      kernels need, per direction (0 = outgoing / SCATTER, 1 = incoming / GATHER), the static tile->row table of the
 *      graph and, for a SPARSE frontier, the exclusive edge offsets of its ids plus the tile->position table. ---- */
int vgl_hip_graph_tile_rows(vgl_hip_graph *g, int direction, const int32_t **d_tile_row, int64_t *ntiles);
int vgl_hip_frontier_advance_plan(vgl_hip_ctx *ctx, vgl_hip_graph *g, vgl_hip_frontier *f, int direction,
                                  const int64_t **d_offs, const int32_t **d_tile_first, int64_t *edges);
/* generate_new_frontier with a USER predicate (the C++ operator class).  The count pass -- predicate, flags, per-tile counts, totals --
 * runs in the caller's translation unit: vgl_k_gnf_count of csrc/vgl_gnf.h instantiated with the user's lambda, launched on the context's
 * stream with the buffers vgl_hip_gnf_begin hands out (plain pointers: the caller never sees the library's internal structures).
 * vgl_hip_gnf_complete waits for that launch (sequence number `seq` from begin, published by the kernel's last workgroup) and does the
 * rest: size / neighbours / sparsity choice (generate_new_frontier.hpp:67-91,113-164) and, for a SPARSE result, the ascending-id
 * compaction -- with the exclusive out-edge offsets of the ids when want_plan != 0, which vgl_hip_frontier_advance_plan(direction 0) reuses.
 * Round 5: the count pass writes the predicate's bits as a BITMAP (V / 8 bytes) instead of V int32 flags, the compaction reads the bitmap, and only a
 * DENSE / ALL_ACTIVE result gets its int32 flags (expanded from the bitmap): a BFS level on RMAT-24 moved 64 MiB of flags out and in again for a frontier
 * of a few thousand ids.  VGL_GNF_INT_FLAGS=1 keeps the flags of every result (the reference's contract to the letter). */
typedef struct {
    int32_t nrows, row_begin;          /* owned rows of the graph handle (generate_new_frontier needs a whole-graph handle) */
    int64_t nvtiles;                   /* 2048-vertex tiles = workgroups of the count launch (256 threads each) */
    const int64_t *out_rowptr;         /* degrees counted into the neighbour total */
    int32_t *vt_cnt, *vt_cnt_off;      /* per-tile counts and their exclusive offsets */
    int64_t *vt_deg, *vt_deg_off;
    uint32_t *ticket;                  /* arrival counters of the launch (the last workgroup scans the tiles) */
    int64_t *counters;                 /* device counter slots */
    volatile int64_t *host_counters;   /* their pinned mirror */
    int32_t *flags;                    /* the frontier's int32 flags for the count pass to write, or NULL (round 5, the default): the pass then leaves only
                                          front_bytes and vgl_hip_gnf_complete writes the flags of a DENSE / ALL_ACTIVE result itself -- the flags of a
                                          SPARSE frontier are not materialised (nothing reads them: every primitive walks its ids) */
    uint8_t *front_bytes;              /* the predicate's bits, byte v >> 3, bit v & 7 (always written by the count pass) */
    int64_t *plan_offs;                /* want_plan: edge-offset array whose terminator the count pass writes, else NULL */
    int64_t seq;                       /* sequence number the launch must publish */
} vgl_hip_gnf_buffers;
int vgl_hip_gnf_begin(vgl_hip_ctx *ctx, vgl_hip_graph *g, vgl_hip_frontier *f, int want_plan, vgl_hip_gnf_buffers *out);
int vgl_hip_gnf_complete(vgl_hip_ctx *ctx, vgl_hip_graph *g, vgl_hip_frontier *f, double dense_threshold, int want_plan, int64_t seq);
/* sums n doubles on the device in a fixed order (the operator class folds its per-workgroup reduce partials with it) */
int vgl_hip_reduce_sum_f64_buffer(vgl_hip_ctx *ctx, int64_t n, const double *d_values, double *result);

/* ---- reduce (reduce_worker_sum, multicore/reduce.hpp:6-60; only REDUCE_SUM is live).
 *      Sums d_values[v] over the frontier's active vertices; deterministic (fixed tree). Synchronises. ---- */
int vgl_hip_reduce_sum_i32(vgl_hip_ctx *ctx, vgl_hip_frontier *f, const int32_t *d_values, int64_t *result);
int vgl_hip_reduce_sum_f32(vgl_hip_ctx *ctx, vgl_hip_frontier *f, const float *d_values, double *result);
/* number of v with a[v] != b[v] (SSSP reduce_changes, shortest_paths.hpp:143-152) */
int vgl_hip_count_not_equal_u32(vgl_hip_ctx *ctx, int32_t n, const void *d_a, const void *d_b, int64_t *result);

/* ---- fused algorithm fast paths (operators of algorithms/{bfs,sssp,pr,cc}) ---- */
typedef struct {
    int32_t levels;            /* frontiers expanded */
    int32_t td_steps, bu_steps;
    int64_t edges_examined;    /* adjacency entries actually read by advance kernels */
    int64_t frontier_total;    /* sum of |F_l| */
    int64_t discovered;        /* vertices reached, incl. source */
    int64_t algorithmic_bytes; /* 8*m_ex + 20*n_front + 4*n_disc + 4*V (+ V/8 per bottom-up level) */
    int64_t td_edges, td_frontier;   /* per-kernel shares for the roofline line: top-down launches */
    int64_t bu_edges, bu_found;      /* bottom-up launches: adjacency entries probed, vertices discovered */
} vgl_hip_bfs_stats;
#define VGL_HIP_BFS_TOP_DOWN 0           /* BFS::fast_vgl_top_down, bfs.hpp:6-51 */
#define VGL_HIP_BFS_DIRECTION_OPT 1      /* + bottom-up steps; switch rule change_state.hpp:100-141 (ALPHA 15, BETA 18) */
int vgl_hip_bfs_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t source, int mode,
                    int32_t *d_levels, vgl_hip_bfs_stats *stats);
/* `count` traversals from HOST source ids one after the other behind one call (the rounds loop of apps/bfs/bfs.cpp:36-50): d_levels is reused
 * and holds the levels of the last source afterwards; stats (optional) has `count` entries.  Stops at the first failing traversal.
 * d_levels may hold anything on entry and belongs to the call until it returns: the first traversal stores every entry, the last one
 * re-initialises the entries a traversal can have written (those below the graph's reach_rows, and the previous source's), and the ones in
 * between re-initialise nothing -- they store their levels above an offset that grows from traversal to traversal and take every smaller value
 * for unvisited.  While the call runs, and after a traversal of it has failed, d_levels therefore holds an internal encoding; on success it holds
 * the levels of the last source (-1 = not reached), as it always did.  VGL_BFS_BATCH_REFILL=1 re-initialises before every traversal. */
int vgl_hip_bfs_run_batch(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *sources, int32_t count, int mode, int32_t *d_levels,
                          vgl_hip_bfs_stats *stats);
/* Optional graph preparation for repeated top-down traversals (the counterpart of the reference's offline graph import,
 * vgl_graph.hpp:57-68): lays the outgoing edges out for the blocked advance (4 bytes per edge kept, a radix sort of the edges once).
 * Afterwards vgl_hip_bfs_run expands the levels that hold at least a tenth of the edges (VGL_BFS_BLOCKED_SHARE) as a blocked pass --
 * one bit per edge travels from the source's block to the destination's, 4.2 bytes per edge streamed -- instead of
 * bfs.hpp:28-36's per-edge probe of levels[dst].  Levels are identical.  The handle must own all rows. */
int vgl_hip_bfs_prepare_blocked(vgl_hip_ctx *ctx, vgl_hip_graph *g);

typedef struct {
    int32_t iterations;
    int64_t edges_relaxed;     /* edges streamed by relax kernels */
    int64_t algorithmic_bytes; /* 12*edges_relaxed + 28*V*iterations */
    int32_t push_steps, pull_steps;   /* super-steps by direction (iterations = their sum) */
} vgl_hip_sssp_stats;
#define VGL_HIP_SSSP_ALL_ACTIVE 0        /* vgl_dijkstra_all_active_push, shortest_paths.hpp:85-163: every iteration streams all edges */
#define VGL_HIP_SSSP_ACTIVE_TILES 1      /* same fixed point, skips edge tiles whose sources did not change */
/* 2 is the bucketed schedule (vgl_hip_sssp_run_delta below; the Python harness uses the number for it) */
#define VGL_HIP_SSSP_PULL 3              /* vgl_dijkstra_all_active_pull, shortest_paths.hpp:169-292: every vertex takes the minimum over its
                                            incoming edges; here a blocked gather / LDS-minimum pass, no scattered stores, no per-edge L2 line */
#define VGL_HIP_SSSP_DIRECTION_OPT 4     /* push over the compacted frontier of the rows that changed (atomic minima) while they own few edges,
                                            pull while they own many; the switch is on the share of edges whose source changed in the last
                                            super-step (VGL_SSSP_PULL_SHARE, 0.2) */
/* Domain of d_weights, for every schedule and plan below: finite, non-negative float32 (+0.0; zero-weight edges and cycles included) whose path
 * sums stay finite.  Nothing else is assumed: weights of 100 and above, denormal weights (kept, not flushed: every candidate is one IEEE
 * round-to-nearest f32 addition, also where values travel through the blocked layouts) and weights 200 binades apart are served like any other.
 * On that domain fl(d + w) is monotone in d and never below d, so the fixed point does not depend on the order of evaluation and the distances
 * of every mode equal the reference's Bellman-Ford and Dijkstra results in every bit; ties change nothing (an update happens only on a strict
 * improvement).  Unreached vertices keep FLT_MAX.  Negative, NaN and infinite weights are outside the contract and are not checked for. */
int vgl_hip_sssp_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_weights, int32_t source, int mode,
                     float *d_dist, vgl_hip_sssp_stats *stats);
/* SSWP::vgl_dijkstra, algorithms/sswp/widest_paths.hpp:5-76 (single-source widest paths): widths[source] = FLT_MAX, others 0;
 * width[dst] = max(width[dst], min(width[src], capacity)) to the fixed point.  Same kernel and modes as vgl_hip_sssp_run with the
 * (max, min) path algebra; only min / max of the inputs occur, so the result is bit-identical to the reference (and to its
 * sequential checker, seq_widest_paths.hpp:5-64).  d_capacities is indexed like the outgoing CSR (global_edge_pos).
 * Domain of d_capacities: non-negative float32 up to and including FLT_MAX, denormals kept.  A capacity of 0 carries nothing: a vertex
 * reached only through such edges keeps width 0, like an unreached one.  A capacity of FLT_MAX passes its source's width on unchanged, so
 * vertices other than the source may end at FLT_MAX. */
/* super-step pieces of the widest-path algorithm for shards (exchange between steps: allreduce(MAX) of the widths) */
int vgl_hip_sswp_init(vgl_hip_ctx *ctx, int32_t V, int32_t source, float *d_widths);
int vgl_hip_sswp_relax_owned(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_capacities, float *d_widths, int *changed);
int vgl_hip_sswp_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_capacities, int32_t source, int mode,
                     float *d_widths, vgl_hip_sssp_stats *stats);
/* The pull steps work on a blocked copy of (outgoing adjacency, edge values) -- vgl_blocked.h -- built once per (graph, weights)
 * like the reference's graph import and reusable for any number of sources; vgl_hip_sssp_run / vgl_hip_sswp_run with mode PULL or
 * DIRECTION_OPT = create + run + destroy.  mode: VGL_HIP_SSSP_PULL or VGL_HIP_SSSP_DIRECTION_OPT.
 * A plan holds a reordered COPY of the edge values: the caller must not rewrite d_weights in place while the plan exists (rebuild the plan
 * after set_all_random or any other writer), and must destroy the plan before the graph handle; a plan is refused for any other handle. */
typedef struct vgl_hip_sssp_pull_plan vgl_hip_sssp_pull_plan;
int vgl_hip_sssp_pull_plan_create(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_weights, vgl_hip_sssp_pull_plan **out);
int vgl_hip_sssp_pull_plan_destroy(vgl_hip_ctx *ctx, vgl_hip_sssp_pull_plan *plan);
/* edges laid out, how many of them as fused tiles (dense pairs of 16384-id blocks: both windows in LDS, 8 bytes per edge streamed instead of
 * 16), bytes one pull pass streams (pad entries included) and bytes the plan keeps resident */
int vgl_hip_sssp_pull_plan_info(vgl_hip_sssp_pull_plan *plan, int64_t *edges, int64_t *fused_edges, int64_t *streamed_bytes_per_pass, int64_t *plan_bytes);
/* one all-edges relaxation through the plan (values of the pass start; the relax of shortest_paths.hpp:123-133 over every edge);
 * *changed = 1 when a distance decreased.  Synchronises. */
int vgl_hip_sssp_pull_pass(vgl_hip_ctx *ctx, vgl_hip_graph *g, vgl_hip_sssp_pull_plan *plan, float *d_dist, int *changed);
int vgl_hip_sssp_run_pull(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_weights, vgl_hip_sssp_pull_plan *plan, int32_t source,
                          int mode, float *d_dist, vgl_hip_sssp_stats *stats);
int vgl_hip_sswp_run_pull(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_capacities, vgl_hip_sssp_pull_plan *plan, int32_t source,
                          int mode, float *d_widths, vgl_hip_sssp_stats *stats);

/* Same operators and bit-identical distances, bucketed schedule (delta-stepping with a light/heavy edge split): light
 * edges (w < delta) of a vertex are relaxed whenever it improves inside the current distance bucket, heavy edges once the
 * bucket has settled.  Cuts the per-edge dist[dst] gathers from ~5 E (Bellman-Ford) to ~1.2 E.  stats->iterations = relax
 * launches (push_steps / pull_steps stay 0).  delta > 0, in the unit of the weights; it only steers the schedule, never the result (for
 * weights in [0,100): 10..25 works well -- advice, not a limit on the weights).  Every positive float is served: w == delta is heavy; a delta
 * above every weight (+inf included: one bucket, every edge light) or not above any (every positive edge heavy) gives a plan with an empty
 * part; a denormal delta makes a bucket of almost every distinct distance -- correct, and slow in proportion.  delta <= 0 or NaN is refused
 * with a status and vgl_hip_last_error() text before d_dist is touched. */
int vgl_hip_sssp_run_delta(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_weights, int32_t source, float delta,
                           float *d_dist, vgl_hip_sssp_stats *stats);
/* The bucketed schedule works on a plan: a copy of the adjacency + weights in which every row's edges are stably
 * partitioned light-first (w < delta), built once per (graph, weights, delta) -- preprocessing in the sense of the
 * reference's graph import, reusable for any number of sources.  run_delta above = create + run + destroy. */
typedef struct vgl_hip_sssp_plan vgl_hip_sssp_plan;
int vgl_hip_sssp_plan_create(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_weights, float delta, vgl_hip_sssp_plan **out);
int vgl_hip_sssp_plan_destroy(vgl_hip_ctx *ctx, vgl_hip_sssp_plan *plan);
int vgl_hip_sssp_run_plan(vgl_hip_ctx *ctx, vgl_hip_graph *g, vgl_hip_sssp_plan *plan, int32_t source, float *d_dist,
                          vgl_hip_sssp_stats *stats);

typedef struct {
    int32_t iterations;
    double ranks_sum;          /* reduce_ranks_sum of the last iteration (pr.hpp:130-134) */
    int64_t algorithmic_bytes; /* (8*E + 28*V) * iterations */
} vgl_hip_pr_stats;
/* vgl_page_rank, pr.hpp:7-149 (f32, d = 0.85, fixed iteration count, reversed-graph definition).
 * d_indeg_noloops: int32[V] = in-degree minus self loops (pr.hpp:31-65), or NULL to have it computed. */
int vgl_hip_pr_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_indeg_noloops, int iterations,
                   float *d_ranks, vgl_hip_pr_stats *stats);
/* Two evaluations of the per-vertex sum (north star: within 1e-6 relative of the reference):
 *   EXACT_ORDER  f32 `+=` chain in adjacency order, bit-identical to seq_page_rank (seq_pr.hpp:81-96); one random L2 line per edge
 *   BLOCKED      contributions gathered from and summed in 128 KiB LDS windows (vgl_blocked.h): 12 B/edge of streamed HBM traffic, no
 *                random line per edge; the sums are exact (64-bit fixed point, rounded to f32 once) and therefore independent of any
 *                order -- they differ from the chain by the CHAIN's rounding error, ~sqrt(n) * 3e-8 for a row of n entries
 *   AUTO         BLOCKED when the graph stores >= 2^25 edges and no row is longer than 256 entries (uniform-random inputs), else
 *                EXACT_ORDER; what vgl_hip_pr_run uses (VGL_PR_MODE=0|1 overrides) */
#define VGL_HIP_PR_EXACT_ORDER 0
#define VGL_HIP_PR_BLOCKED 1
#define VGL_HIP_PR_AUTO 2
int vgl_hip_pr_run_mode(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_indeg_noloops, int iterations, int mode,
                        float *d_ranks, vgl_hip_pr_stats *stats);
/* Graph preparation for PageRank / Shiloach-Vishkin (the counterpart of the reference's offline import): builds NOW what the first
 * vgl_hip_pr_run / vgl_hip_cc_run would otherwise build inside its first call -- the blocked layout (a radix sort of the edges, tens of ms
 * for 10^9 edges plus the allocations) or the hub schedule of the ordered pull.  *resolved_mode (optional): what AUTO resolved to.  The
 * default entry point vgl_hip_pr_run uses AUTO: bit-identical to seq_page_rank below 2^25 stored edges or when a row is longer than 256
 * entries, exact per-vertex sums (<= 1e-6 of the chain on such graphs, NOT bit-identical) otherwise; pass VGL_HIP_PR_EXACT_ORDER to
 * vgl_hip_pr_run_mode for the reference's evaluation order at any size. */
int vgl_hip_pr_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int mode, int *resolved_mode);
int vgl_hip_cc_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g);
/* Graph preparation for the path algorithms (Bellman-Ford / widest paths; counterpart of the reference's import, which derives every edge-array layout
 * from one permutation, csr_edges_array.hpp:31-40): builds the blocked STRUCTURE of the outgoing CSR once per graph -- one radix sort of the edges by
 * block pair, the CSR position behind every value slot kept.  Afterwards a pull plan for ANY weights array (vgl_hip_sssp_pull_plan_create) is one
 * gather pass, and vgl_hip_sssp_run(ALL_ACTIVE) -- the reference's schedule, every edge in every super-step -- runs as blocked passes (same fixed
 * point, same f32 bits).  Needs a handle that owns all rows. */
int vgl_hip_sssp_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g);

typedef struct {
    int32_t hook_passes;
    int64_t algorithmic_bytes; /* (8*E + 12*V) per hook pass + 12*V per jump pass */
} vgl_hip_cc_stats;
/* SCC::vgl_forward_backward, algorithms/scc/scc.hpp (checker SCC::seq_tarjan, seq_scc.hpp): strongly connected components of a
 * directed graph.  d_comp[v] = smallest vertex id of v's component: the canonical form of the partition (the reference's labels are
 * arbitrary counters and its test compares partitions, verify_results.h equal_components).  Needs the incoming CSR. */
typedef struct {
    int32_t trim_rounds;             /* vertex passes that removed trivial components */
    int32_t forward_backward_steps;  /* pivot reach steps (0 or 1: the big component) */
    int32_t colour_rounds;           /* colour-class rounds for the remaining components */
    int32_t edge_passes;             /* all-edges passes of those rounds (inactive tiles skipped) */
} vgl_hip_scc_stats;
int vgl_hip_scc_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_comp, vgl_hip_scc_stats *stats);

/* HITS::vgl_hits, algorithms/hits/hits.hpp:5-100 (f64, apps/hits/hits.cpp:13): auth = hub = 1, then `steps` times
 *   auth[v] = sum of hub over the in-neighbours, auth /= ||auth||_2, hub[v] = sum of auth over the out-neighbours, hub /= ||hub||_2.
 * Per-vertex sums run in adjacency order (the sequential checker's order, hits.hpp:117-160); norms are folded in a fixed order.
 * Needs the incoming CSR.  Deterministic; agrees with seq_hits to ~1e-15 relative. */
int vgl_hip_hits_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int steps, double *d_auth, double *d_hub);

/* vgl_shiloach_vishkin, shiloach_vishkin.hpp:7-88: labels = min id that reaches each vertex */
int vgl_hip_cc_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_comp, vgl_hip_cc_stats *stats);
/* Same labels for SYMMETRIC graphs only (every edge stored in both directions, as the reference's cc app builds its input,
 * apps/cc/cc.cpp:24-36 UNDIRECTED_GRAPH): the fixed point of the hook/jump loop is then "smallest id of the connected component",
 * which a min-id union-find reaches without sweeping all edges repeatedly -- two sampled neighbours per vertex, then only the
 * rows outside the largest tree look at their edges.  The caller vouches for the symmetry; on a directed graph the labels
 * are those of the weakly-connected components of the stored edges, NOT vgl_hip_cc_run's.  stats->hook_passes counts the
 * link passes (sampling rounds + 1), algorithmic_bytes what those passes had to touch. */
int vgl_hip_cc_run_symmetric(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_comp, vgl_hip_cc_stats *stats);

/* Label propagation: the AlwaysActive GPU path of LabelPropagation::gpu_lp (algorithms/lp/gpu/lp_gpu.cu:185-420 with
 * active_conditions.cuh:6-37), stated so that a sequential restatement reproduces it bit for bit:
 *   N(v)   v's stored adjacency in `direction` (0 = OUT, 1 = IN).  Every stored entry counts once: multi-edges with their multiplicity,
 *          a self-loop with v's own label (the reference's gather, lp_gpu.cu:290-298).
 *   L0     d_init[v], or -- d_init == NULL -- v's id in the graph's numbering (callers of a renumbered graph pass its stored -> original
 *          table, so that the answer does not depend on the numbering).  Labels are arbitrary int32 values, INT32_MIN / INT32_MAX included.
 *   step   synchronous: every read of iteration t sees L_{t-1}.  N(v) empty: L_t[v] = L_{t-1}[v].  Otherwise L_t[v] is the label with
 *          the highest count in N(v); a tie goes to the LARGEST label (the reference sorts each segment ascending and reduces with
 *          `w_a > w_b ? a : b`, lp_gpu.cu:374, which keeps the rightmost maximum whatever the association order).
 *   stop   after the first iteration that changes no label (converged = 1; that iteration is counted), or after max_iterations
 *          (the reference's default 20, lp.h:10).  The reference always runs to the cap (it sets updated[0] = 1 unconditionally,
 *          lp_gpu.cu:414); a fixed point is stable, so the labels are the same.  A synchronous LP can oscillate (K2,2): the cap decides.
 * Not reproduced: seq_lp (vertex shuffle and coin-flip ties, seq_lp.hpp:36,71) and the heuristic active conditions.
 * mode: ALL_ACTIVE evaluates every row every iteration; FRONTIER evaluates only the rows with a neighbour that changed in the iteration
 * before (exact: such a row keeps its label), found by pushing the changed vertices over the REVERSE CSR -- the incoming one for OUT, the
 * outgoing one for IN, or the CSR in use itself when the caller vouches that it is symmetric; AUTO = FRONTIER when that reverse is
 * available, else ALL_ACTIVE.  All modes give the same labels, iteration counts and changed counts.
 * changed_history (host, may be NULL): entry t = vertices whose label changed in iteration t, for t < stats->iterations.
 * Fails for a sharded handle, IN without the incoming CSR, FRONTIER without a reverse CSR, max_iterations < 0.
 * vgl_hip_lp_prepare builds the degree classes of `direction` (and the push schedule of its reverse) now, outside any timing; the
 * first run would build them otherwise.  They are cached on the graph handle and freed with it. */
#define VGL_LP_ALL_ACTIVE 0
#define VGL_LP_FRONTIER 1
#define VGL_LP_AUTO 2
typedef struct {
    int32_t iterations;          /* iterations run, the last one (no change) included when converged */
    int32_t converged;
    int32_t frontier_steps;      /* iterations that evaluated a frontier instead of every row */
    int64_t changed_last;        /* vertices changed by the last iteration */
    int64_t rows_processed;      /* rows (with at least one entry) evaluated, summed over the iterations */
    int64_t edges_examined;      /* their entries: iterations * E when every iteration evaluates every row */
    int64_t algorithmic_bytes;   /* 16*V + 8*E per all-active iteration (row offsets, label read / write; adjacency, gathered labels) + frontier upkeep */
} vgl_hip_lp_stats;
int vgl_hip_lp_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int direction);
int vgl_hip_lp_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int direction, int mode, int symmetric, int max_iterations, const int32_t *d_init,
                   int32_t *d_labels, int64_t *changed_history, vgl_hip_lp_stats *stats);

/* Triangle counting (`tri`; `tc` in this library is transitive closure).  The reference has none, so this comment is the contract:
 *   input     any vgl_hip_graph that owns all rows (not a sharded handle).  Only the stored OUTGOING CSR is read; the incoming CSR is not needed.
 *   graph     the simple undirected graph underlying the stored entries: u ~ v iff u != v and at least one of (u, v), (v, u) is stored.
 *             Self-loops are ignored; multi-edges and an edge stored both ways count once.  A directed 3-cycle is one triangle.
 *   triangles number of unordered vertex triples that are pairwise adjacent (int64, host).
 *   d_per_vertex[v]  number of triangles that contain v (int64, device, may be NULL), in the graph's own numbering.  Sum over v = 3 * triangles.
 *   d_degree[v]      degree of v in that simple undirected graph (int32, device, may be NULL).  The local clustering coefficient
 *             2 t[v] / (d[v] (d[v] - 1)), 0 where d < 2, is derived by the callers in float64; there is no float on the device.
 *   The answer does not depend on the vertex order used internally, on the VGL_TRI_* thresholds or on the order of the entries in a row.
 * Method: every undirected edge is given to its endpoint that is LOWER in the total order (stored out-degree [+ in-degree when the incoming CSR
 * exists], id) -- the oriented CSR, rows ascending by vertex id, built once by vgl_hip_tri_prepare (or by the first run), cached on the handle and
 * freed with it -- and triangles = sum over oriented edges (a, b) of |N+(a) & N+(b)|.
 * stats: undirected_edges = E' (simple undirected edges = entries of the oriented CSR); intersections = oriented edges evaluated = E';
 * elements_examined = entries of second lists examined, exactly: for an edge (a, b) of a light row min(d+(a), d+(b)) (the shorter list is walked, each
 * element searched in the longer one), of a table row d+(b) (N+(b) is streamed once against the LDS set of N+(a)), of a huge row d+(b) times the row's
 * chunks, ceil(d+(a) / VGL_TRI_HUGE_CHUNK); algorithmic_bytes = 8 V + 4 E' + 4 elements_examined (the oriented CSR read once + every examined
 * element); rows_* = rows with at least one oriented entry per class.  prepared_now = 1 when this call built the oriented CSR.
 * Fails for a sharded handle and for triangles == NULL. */
typedef struct {
    int64_t triangles;
    int64_t undirected_edges;
    int64_t intersections;
    int64_t elements_examined;
    int64_t algorithmic_bytes;
    int32_t max_oriented_degree;
    int32_t prepared_now;
    int64_t rows_light, rows_table, rows_huge;
} vgl_hip_tri_stats;
int vgl_hip_tri_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g);
int vgl_hip_tri_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int64_t *triangles, int64_t *d_per_vertex, int32_t *d_degree, vgl_hip_tri_stats *stats);

/* Betweenness centrality (`bc`, Brandes' algorithm).  The reference has none, so this comment is the contract:
 *   graph     the stored DIRECTED, unweighted graph of a handle that owns all rows.  Every stored entry is an edge of its own: multi-edges count with
 *             their multiplicity in the path counts (as in label propagation's contract); a self-loop is never on a shortest path and has no effect.
 *   per source s (levels exactly as vgl_hip_bfs_run writes them: source 1, unreached -1; below d(s, v) = levels[v] - 1 counts edges):
 *             sigma_s[s] = 1, sigma_s[v] = sum over the stored entries (u, v) with d(s, u) = d(s, v) - 1 of sigma_s[u]; unreached: sigma = 0;
 *             delta_s[v] = sum over the stored entries (v, w) with d(s, w) = d(s, v) + 1 of sigma_s[v] / sigma_s[w] * (1 + delta_s[w]),
 *             evaluated as sigma_s[v] * (sum of coef[w]), coef[w] = (1 + delta_s[w]) / sigma_s[w]; unreached: delta = 0.
 *   result    d_bc[v] = sum over the sources s != v of delta_s[v]: float64, in the graph's own numbering, directed, unnormalised, endpoints not
 *             counted.  accumulate = 0 overwrites d_bc, 1 adds to what it holds.  On a symmetric graph every unordered pair is counted twice; halving,
 *             the V / k rescaling of a source sample and any normalisation are the callers' business, in float64.
 *   types     sigma, delta, bc are float64; there is no float32 on this path.  sigma is exact while below 2^53 and rounded above;
 *             stats->sigma_inexact counts the sources whose largest sigma reached 2^53.
 *   directions the forward sweep (sigma) reads the incoming CSR, the backward sweep (delta) the outgoing one.  symmetric = 1: the caller vouches that
 *             the stored graph is symmetric, and the outgoing CSR serves both (the rule of vgl_hip_lp_run).
 *   determinism no floating-point atomics: both sweeps are pulls, every value has one writer per source and a summation shape fixed by the row's
 *             length and the VGL_BC_* switches.  Two runs of the same call on the same handle under the same switches give bit-identical d_bc.
 *   sources   host array of `count` vertex ids in the graph's numbering, run one after the other (a repeated source counts again).
 *   d_levels, d_sigma, d_delta (device, V each, optional): the LAST source's arrays.
 * Method: per source the levels come from the traversal of vgl_hip_bfs_run; the reached vertices are bucketed by (level, row class) once, so that the two
 * sweeps cost O(reached vertices + their entries) and not O(depth * V); rows are split by length into classes (VGL_BC_SHORT 32: 8 lanes per row,
 * VGL_BC_WAVE 1024: a wavefront, VGL_BC_WG 32768: a workgroup, longer: one workgroup per VGL_BC_CHUNK 16384 entries and a fold in chunk order).
 * The classes of both directions are built by vgl_hip_bc_prepare or the first run, cached on the graph handle and freed with it.
 * stats: sources = traversals run; max_depth = largest d(s, v); levels_total = sum over the sources of (deepest d + 1), the frontiers a traversal
 * expands; reached_total = vertices reached, source included; edges_forward = entries of the forward CSR in the rows of the reached non-source
 * vertices, edges_backward = outgoing entries of the reached vertices that are not on the last level: exactly the rows the sweeps are launched over;
 * algorithmic_bytes = per source the traversal's own model + (10 V + 4 reached) per order (one order per direction: levels and class read twice,
 * the order written) + 28 (reached - 1) + 52 reached for the per-row reads and writes of the two sweeps + 8 per entry walked (adjacency and
 * the endpoint's level; the 8-byte gathers of matching entries are left out: a lower bound).
 * Fails, before d_bc is written: a sharded handle, no incoming CSR without symmetric = 1, a source outside [0, V), count < 0, d_bc == NULL. */
typedef struct {
    int32_t sources;            /* traversals run */
    int32_t max_depth;          /* largest d(s, v) over all sources */
    int32_t sigma_inexact;      /* sources whose largest sigma reached 2^53 */
    int32_t prepared_now;       /* this call built row classes */
    int64_t levels_total;       /* sum over sources of frontiers expanded */
    int64_t reached_total;      /* sum over sources of vertices reached, source included */
    int64_t edges_forward;      /* forward-CSR entries of reached non-source vertices, summed over sources: exact */
    int64_t edges_backward;     /* outgoing entries of reached vertices that are not on the last level, summed: exact */
    int64_t algorithmic_bytes;
} vgl_hip_bc_stats;
int vgl_hip_bc_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int symmetric);
int vgl_hip_bc_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *sources, int32_t count, int symmetric, int accumulate, double *d_bc,
                   int32_t *d_levels, double *d_sigma, double *d_delta, vgl_hip_bc_stats *stats);

/* k-core decomposition (`kcore`): core numbers and the degeneracy.  The reference has none, so this comment is the contract:
 *   input     any handle that owns all rows; only the stored outgoing CSR is read.
 *   graph     the simple undirected graph of triangle counting's contract: u ~ v iff u != v and at least one of (u, v), (v, u) is stored.
 *             Self-loops are ignored; multi-edges and an edge stored both ways count once.
 *   result    d_core[v] (int32, device, V entries, required), in the graph's own numbering: the largest k such that v lies in a subgraph in which
 *             every vertex has degree >= k.  An isolated vertex gets 0.
 *   k_limit   > 0: the peel stops once k reaches it and every remaining vertex gets k_limit, so that d_core = min(core, k_limit) -- one k-core
 *             ({v : d_core[v] >= k}) without paying for the denser tail.  0: the whole decomposition.  Negative: an error.
 *   d_degree  (int32, device, V entries, optional): the degree in that simple graph (the meaning of vgl_hip_tri_run's d_degree).
 *   The answer does not depend on the vertex order used internally, on the VGL_KCORE_* switches, on the order of the entries in a row or on the
 *   order in which the atomics land: core numbers are integers and unique.
 * Method: the symmetric simple CSR (row offsets int64, adjacency int32, degrees int32) is built once by vgl_hip_kcore_prepare (or by the first run) from
 * the sorted, deduplicated 64-bit keys u << 32 | v and v << 32 | u of the stored entries -- in pieces of consecutive rows when the keys would need more
 * scratch than VGL_KCORE_SORT_CAP_MB -- cached on the handle and freed with it.  The peel is level-synchronous on a working copy of the degrees: for
 * the current k the vertices with degree <= k form the first frontier; an expanded vertex gets core = k and, for every neighbour u whose degree is
 * still above k, old = atomicSub(&deg[u], 1): the one thread that sees old == k + 1 appends u to the next frontier, a thread that sees old <= k puts its
 * decrement back.  When the frontier is empty k becomes the smallest remaining degree (a device reduction: no walk through empty shells).  Frontier
 * rows are split by length (VGL_KCORE_SHORT 32: 8 lanes per row, VGL_KCORE_WAVE 1024: a wavefront, longer: one workgroup per VGL_KCORE_CHUNK 16384
 * entries); frontiers of at most 2048 vertices and VGL_KCORE_SMALL (8192; 0 = off) entries run several per launch in ONE workgroup.
 * stats, all exact and the same on every run (sub_rounds depends on the VGL_KCORE_SMALL switch only through how the work is batched, not in value):
 * degeneracy = the largest value written to d_core; rounds = values of k the peel visited (a full run: the number of distinct core values);
 * sub_rounds = frontiers expanded; undirected_edges = E'; edges_examined = adjacency entries walked (<= 2 E': every vertex is expanded at most
 * once); max_degree = the longest row of the symmetric CSR; prepared_now = this call built the symmetric CSR;
 * algorithmic_bytes = 20 V (row offsets read once, degrees copied, core written) + 8 per entry walked (the adjacency entry and the neighbour's
 * degree); the per-k scans of the degree array and the atomics' write traffic are left out: a lower bound.
 * Fails, before d_core is written: a sharded handle, d_core == NULL, k_limit < 0. */
typedef struct {
    int32_t degeneracy;         /* largest value written to d_core */
    int32_t rounds;             /* values of k visited */
    int32_t max_degree;         /* longest row of the symmetric CSR */
    int32_t prepared_now;       /* this call built the symmetric CSR */
    int64_t sub_rounds;         /* frontiers expanded */
    int64_t undirected_edges;   /* E' */
    int64_t edges_examined;     /* adjacency entries walked */
    int64_t algorithmic_bytes;
} vgl_hip_kcore_stats;
int vgl_hip_kcore_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g);
int vgl_hip_kcore_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t k_limit, int32_t *d_core, int32_t *d_degree, vgl_hip_kcore_stats *stats);

/* k-truss decomposition (`ktruss`): the truss number of every edge.  The reference has none, so this comment is the contract:
 *   input     any handle that owns all rows; only the stored outgoing CSR is read.
 *   graph     the simple undirected graph of triangle counting's contract: u ~ v iff u != v and at least one of (u, v), (v, u) is stored.
 *   edges     the E' undirected edges {lo < hi} are numbered 0 .. E' - 1 in ascending (lo, hi) order of the graph's own vertex numbering.  This is the
 *             library's edge numbering of that graph: d_edge_u[i] = lo, d_edge_v[i] = hi of edge i.  E' >= 2^31 is an error.
 *   support   support(e) = number of triangles of that graph that contain e; d_support receives this INITIAL support.  Sum = 3 * triangles.
 *   result    d_truss[e] (int32, device, E' entries, required): the largest k such that e lies in a subgraph in which every edge is in at least k - 2
 *             triangles of that subgraph.  An edge in no triangle has truss 2; every edge of K_n has truss n.
 *   k_limit   0: the whole decomposition.  >= 2: the peel stops when k reaches it and every remaining edge gets k_limit, so that
 *             d_truss = min(truss, k_limit).  1 or negative: an error.
 *   The answer does not depend on the vertex order used internally, on any VGL_KTRUSS_* switch, on the order of the entries in a row or on the order in
 *   which the atomics land: truss numbers are integers and unique.
 * Method: vgl_hip_ktruss_prepare (or the first run) takes the handle's symmetric simple CSR (built if the handle has none; kcore, ktruss and msf share it) and adds
 * eid (int32 per adjacency slot: the edge id) and the endpoint arrays, cached on the handle and freed with it; *undirected_edges (host, may be NULL)
 * receives E'.  A run computes the initial support in one pass without atomics on the supports (per edge the SHORTER of the two full rows is walked,
 * each entry searched in the longer), then peels level-synchronously: k = the smallest support of an alive edge + 2 (a device reduction, no walk through
 * empty levels); the alive edges with support <= k - 2 are the first frontier of k; an expanded edge gets truss k, and every triangle it is in whose
 * other two edges have not been removed in an earlier sub-round is destroyed exactly once: if neither of the two is in the current frontier both are
 * decremented, if exactly one is the third edge is decremented by the frontier edge of the smaller id, if both are nothing is.  A decrement is
 * old = atomicSub(&support[e], 1): old == k - 1 appends e to the next frontier, old <= k - 2 is put back.  Edges are split by the length of the shorter
 * row: <= VGL_KTRUSS_SHORT (32) 8 lanes per edge, <= VGL_KTRUSS_WAVE (1024) a wavefront, longer a workgroup.
 * stats, all exact and the same on every run:
 *   max_truss = the largest value written to d_truss (0 when E' = 0); rounds = values of k the peel visited (= the distinct truss values below
 *   k_limit); sub_rounds = frontiers expanded; max_support = the largest initial support; prepared_now = this call built eid and the endpoint arrays;
 *   undirected_edges = E'; triangles = sum of the initial supports / 3;
 *   support_elements = adjacency entries the support pass walked = sum over all edges (u, v) of min(d(u), d(v)), d = the degree in the simple graph
 *   (the shorter row is walked once, whatever the class; the probes of the binary search in the longer row are not counted);
 *   peel_elements = adjacency entries the peel walked = the same sum over the edges the peel expanded (every edge, or those of truss < k_limit);
 *   algorithmic_bytes = 28 E' (support pass: two endpoints read, the support written; peel: two endpoints read, truss and the sub-round stamp written)
 *   + 4 (support_elements + peel_elements) (every walked entry once); the search probes, the edge ids, stamps and supports read per triangle, the
 *   atomics' traffic and the per-k scans are left out: a lower bound.
 * Fails, before anything is written: a sharded handle, d_truss == NULL, one of d_edge_u / d_edge_v without the other, k_limit == 1 or < 0. */
typedef struct {
    int32_t max_truss;          /* largest value written to d_truss; 0 when E' = 0 */
    int32_t rounds;             /* values of k visited */
    int32_t max_support;        /* largest initial support */
    int32_t prepared_now;       /* this call built the edge ids */
    int64_t sub_rounds;         /* frontiers expanded */
    int64_t undirected_edges;   /* E' */
    int64_t triangles;
    int64_t support_elements;   /* entries walked by the support pass */
    int64_t peel_elements;      /* entries walked by the peel */
    int64_t algorithmic_bytes;
} vgl_hip_ktruss_stats;
int vgl_hip_ktruss_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int64_t *undirected_edges);
int vgl_hip_ktruss_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t k_limit, int32_t *d_edge_u, int32_t *d_edge_v, int32_t *d_truss, int32_t *d_support,
                       vgl_hip_ktruss_stats *stats);

/* Minimum spanning forest (`msf`): Boruvka on the weighted simple undirected graph.  The reference has none, so this comment is the contract:
 *   input     any handle that owns all rows; only the stored outgoing CSR is read.  d_weights: float32, device, one per stored outgoing entry in
 *             the order of the outgoing CSR, exactly as vgl_hip_sssp_run takes them (may be NULL only when nothing is stored).
 *   graph     the simple undirected graph of triangle counting's contract: u ~ v iff u != v and at least one of (u, v), (v, u) is stored.
 *   weight    of the undirected edge {lo, hi}: the smallest weight over all stored entries (lo, hi) and (hi, lo) -- a multi-edge counts with its
 *             lightest copy.  Loops are ignored, their weights included.
 *   edges     carry the library's edge numbering of vgl_hip_ktruss_run (ascending (lo, hi) in the graph's own vertex numbering, E' < 2^31); it is
 *             taken from the handle's k-truss cache (built if absent, shared afterwards), there is no second numbering.
 *   order     edges are totally ordered by (weight, edge id); weights compare as numbers: -0.0 equals +0.0, -inf and +inf are allowed.  The order is
 *             strict, so the forest is unique: e is in it iff e is not the largest edge of any cycle.
 *   NaN       a NaN among the weights of non-loop entries is an error (the message names `weights`), reported before any output is written.
 *   outputs   d_in_forest (uint8, E' entries, required): 1 / 0;  d_edge_weight (float32, E', optional): the folded weight;  d_edge_u / d_edge_v
 *             (int32, E', optional, both or neither): lo, hi as in k-truss;  d_component (int32, V, optional): the smallest vertex id, in the
 *             graph's own numbering, of the vertex's component of that graph -- an isolated vertex is its own component.
 *   rounds    the number of synchronous Boruvka rounds that added an edge, under this rule: in a round every current component that has a crossing
 *             edge picks its smallest crossing edge in the order above; all picked edges join the forest; the components are merged along all of
 *             them to completion before the next round.  With the strict order this is a function of the graph and the weights alone: rounds is
 *             exact, 0 when E' = 0, at most ceil(log2 V).
 *   The answer does not depend on the order of the entries in a row, on any VGL_MSF_* switch or on the order in which the atomics land.
 * Method: vgl_hip_msf_prepare (or the first run) takes the handle's symmetric simple CSR and the edge ids of its slots (built if the handle has none; shared with kcore and ktruss)
 * and adds slot_eid, int32 per STORED outgoing entry: its undirected edge, -1 for a loop (a binary search of the entry in its symmetric row); cached on
 * the handle and freed with it; *undirected_edges (host, may be NULL) receives E'.  Structure is per graph, values are per weights: a run folds the
 * weights in one streaming pass (the float as an order-preserving uint32 -- -0.0 canonicalised, the sign bit flipped, negatives complemented -- and
 * an integer atomicMin per entry on wkey[edge]; the same pass counts the NaNs).  A round: the live rows, one kernel per row class (<= VGL_MSF_SHORT
 * (32): 8 lanes per row, <= VGL_MSF_WAVE (1024): a wavefront, longer: one workgroup per VGL_MSF_CHUNK (16384) entries), keep per row the smallest
 * key  wkey << 32 | edge id  over the entries that lead into another component and make one 64-bit atomicMin on best[component] (skipped when the
 * slot already holds a smaller key; the short rows of a wave that share a component go as one); a row without a crossing entry leaves the live list
 * for good.  Every root c with a pick e hooks to the component d at the far end -- unless d picked e as well and c < d, then c stays a root --
 * sets in_forest[e] and counts the edge (so an edge is counted once); parents are chased to the roots into a second array, the labels rewritten, and
 * the host reads the round's totals once from the pinned mirror.  The loop ends on a round with no pick.
 * stats, all exact and the same on every run:
 *   rounds as above; prepared_now = this call built slot_eid; forest_edges = edges in the forest; components = V - forest_edges;
 *   undirected_edges = E';  entries_walked = adjacency entries the min-edge passes walked = the row lengths of the live rows, summed over the rounds
 *   (for E' > 0: 2 E' <= entries_walked <= (rounds + 1) 2 E');
 *   algorithmic_bytes = 8 E (fold: slot_eid and the weight of every stored entry) + 5 E' (wkey and in_forest written) + 12 entries_walked (the
 *   adjacency entry, its edge id and the far end's component) + 20 V rounds (hook: component and best read; relabel: component read and written);
 *   the keys of the crossing entries, the atomics' traffic, the live lists and the last, empty round's vertex passes are left out: a lower bound; 0 when E' = 0 (no pass runs);
 *   total_weight = the float64 sum of the forest edges' float32 weights, without floating-point atomics and in a shape fixed by E' alone (per-workgroup
 *   partials stored, then one workgroup sums them in index order): bit-identical from run to run.
 * Fails, before anything is written: a sharded handle, d_in_forest == NULL, d_weights == NULL while entries are stored, one of d_edge_u / d_edge_v
 * without the other, a NaN weight on a non-loop entry. */
typedef struct {
    int32_t rounds;             /* Boruvka rounds that added an edge */
    int32_t prepared_now;       /* this call built slot_eid */
    int64_t forest_edges;
    int64_t components;         /* V - forest_edges */
    int64_t undirected_edges;   /* E' */
    int64_t entries_walked;     /* adjacency entries walked by the min-edge passes */
    int64_t algorithmic_bytes;
    double total_weight;        /* float64 sum of the forest edges' float32 weights */
} vgl_hip_msf_stats;
int vgl_hip_msf_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int64_t *undirected_edges);
int vgl_hip_msf_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_weights, int32_t *d_edge_u, int32_t *d_edge_v, float *d_edge_weight,
                    uint8_t *d_in_forest, int32_t *d_component, vgl_hip_msf_stats *stats);

/* Multi-source BFS (`msbfs`, bit-parallel: Then et al., VLDB 2014) and the per-source sums that closeness, harmonic centrality and eccentricity are
 * made of.  The reference has none, so this comment is the contract:
 *   graph     the stored DIRECTED, unweighted graph of a handle that owns all rows.  Multi-edges and self-loops have no effect on distances.
 *   direction 0: d(s, v) counts edges along stored outgoing entries, as vgl_hip_bfs_run does.  1: distances run along incoming entries, so d is the
 *             distance from v to s.  symmetric = 1: the caller vouches that the stored graph is symmetric, and the outgoing CSR serves everything
 *             (the rule of vgl_hip_lp_run and vgl_hip_bc_run).
 *   sources   host array of `count` vertex ids in the graph's numbering.  Batch k is sources[64 k .. 64 k + 63], in the given order; the last batch
 *             may be partial.  A repeated source is a traversal of its own: two bits may start on one vertex.
 *   per-source outputs (device arrays of `count` entries in source order; each may be NULL, but at least one output must be given):
 *             d_reached   int64: the number of vertices with a finite d, the source included;
 *             d_dist_sum  int64: the sum over those vertices of d(s, v);
 *             d_ecc       int32: the largest finite d;
 *             d_harmonic  float64:  h = 0; for d = 1 .. ecc ascending: h = h + (double)n_d / (double)d,  n_d = the number of vertices at distance d.
 *                         Each value has one writer, takes one IEEE division and one addition per level in that fixed order, and no floating-point
 *                         atomics; the library is built with -ffp-contract=off and without fast-math, so the value is bit-identical from run to
 *                         run and to the same loop in numpy float64.
 *   d_levels  (optional) count x V int32, source-major, indexed with int64: row j holds exactly what vgl_hip_bfs_run writes for sources[j] (the source
 *             gets 1, unreached vertices get -1).
 *   Closeness, the Wasserman-Faust scaling and any other normalisation are the callers' business, in float64 (the rule of tri's clustering coefficient).
 * Method: every vertex carries 64-bit words (seen, cur, nxt: 24 bytes per vertex), bit b = source b of the batch, and the frontier is also kept as
 * vertex lists, one per row class of the traversal direction (VGL_MSBFS_SHORT 32: 8 lanes per row, VGL_MSBFS_WAVE 1024: a wavefront, longer: one
 * workgroup per VGL_MSBFS_CHUNK 16384 entries).  A push level walks the listed rows: add = cur[v] & ~seen[w] goes to nxt[w] by a 64-bit atomicOr, and
 * the lane that found the word empty lists w.  A pull level walks all rows of the reverse CSR: want = live bits & ~seen[v]; a row with want == 0 is not
 * read, the others OR cur[u] over their entries until want is covered.  A level is a pull iff the reverse CSR of the traversal direction is there
 * (the incoming CSR for direction 0, the outgoing for 1, the outgoing under symmetric) and the frontier's entries exceed VGL_MSBFS_PULL_SHARE (0.05)
 * of E; VGL_MSBFS_MODE = auto | push | pull forces the schedule (pull without a reverse CSR is an error); all give identical outputs.  Settle runs over
 * the new lists only, counts per source with wave-64 ballots, and a 64-thread kernel folds the counts into the outputs and publishes the level's
 * totals: one host read per level.  The row classes per direction are built by vgl_hip_msbfs_prepare or the first run, cached on the handle and freed
 * with it.
 * stats: sources = traversals run; batches = ceil(count / 64); max_depth = the largest ecc; levels_total = sum over the batches of (largest ecc in the
 * batch + 1): every level with a non-empty frontier is expanded, the last one included; levels_push + levels_pull = levels_total;
 * reached_total = sum of reached; edges_push = sum over the push levels of the traversal-direction degree of every vertex whose frontier word is
 * non-zero: exact, and a function of the graph and the sources alone when the schedule is forced to push; edges_pull = entries examined in pull
 * levels (rows exit early: not pinned); prepared_now = this call built row classes;
 * algorithmic_bytes = 24 V per batch (the words cleared) + 12 per entry walked (the adjacency entry and one word of its far end) + 12 V per pull
 * level (the row list and the seen word of every vertex) + 76 per (frontier vertex, level) pair (its list entry written and read twice, nxt read,
 * seen read and written, cur cleared, its row bounds read by the level and by settle, its class) + with d_levels 4 count V + 4 reached_total;
 * the atomics' traffic is left out: a lower bound.
 * Fails, before any output is written: a sharded handle, direction 1 without an incoming CSR and without symmetric = 1, a source outside [0, V),
 * count < 0, all outputs NULL.  direction 0 without an incoming CSR does not fail: it runs push-only.  count == 0 succeeds and writes nothing. */
typedef struct {
    int32_t sources;            /* traversals run */
    int32_t batches;            /* words of 64 sources */
    int32_t max_depth;          /* largest ecc over all sources */
    int32_t prepared_now;       /* this call built row classes */
    int32_t levels_push;        /* levels expanded top-down */
    int32_t levels_pull;        /* levels expanded bottom-up */
    int64_t levels_total;       /* sum over batches of frontiers expanded */
    int64_t reached_total;      /* sum over sources of vertices reached, source included */
    int64_t edges_push;         /* entries of the frontier vertices of the push levels: exact */
    int64_t edges_pull;         /* entries examined by the pull levels */
    int64_t algorithmic_bytes;
} vgl_hip_msbfs_stats;
int vgl_hip_msbfs_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int direction, int symmetric);
int vgl_hip_msbfs_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *sources, int32_t count, int direction, int symmetric, int64_t *d_reached,
                      int64_t *d_dist_sum, int32_t *d_ecc, double *d_harmonic, int32_t *d_levels, vgl_hip_msbfs_stats *stats);

/* Biconnectivity (`bicc`): bridges, cut vertices (articulation points), biconnected components (blocks) and 2-edge-connected components of the simple
 * undirected graph.  The reference has none, so this comment is the contract:
 *   input     any handle that owns all rows; only the stored outgoing CSR is read.
 *   graph     the simple undirected graph of triangle counting's contract: u ~ v iff u != v and at least one of (u, v), (v, u) is stored.  Loops,
 *             parallel entries and antiparallel entries do not matter: an edge stored twice is still a bridge if it is one.
 *   edges     carry the library's edge numbering of vgl_hip_ktruss_run (ascending (lo, hi) in the graph's own vertex numbering, E' < 2^31), taken from
 *             the handle's cache (built if absent, shared with ktruss and msf afterwards).  The blocks are a partition of exactly these E' edges.
 *   outputs   (device; each may be NULL, but at least one must be given; the edge arrays are sized by the caller like k-truss's: E' <= stored entries)
 *             d_edge_u / d_edge_v      int32, E', both or neither: lo, hi of edge i;
 *             d_bridge                 uint8, E': 1 iff removing the edge disconnects its component;
 *             d_edge_component         int32, E': the block of the edge = the SMALLEST EDGE ID in that block; a bridge is a block of its own, its
 *                                      label is its own id;
 *             d_articulation           uint8, V: 1 iff removing the vertex disconnects its component; an isolated vertex is no cut vertex;
 *             d_two_edge_component     int32, V: the SMALLEST VERTEX ID of the vertex's component of (graph minus bridges); an isolated vertex is a
 *                                      component of its own.
 *             All ids are in the graph's own numbering.
 *   The answer does not depend on any VGL_BICC_* switch, on the order of the entries in a row, on which parent a vertex gets in the forest or on the
 *   order in which the atomics land: every output is an integer and unique.
 * Method: the Tarjan-Vishkin reduction on a rooted BFS forest of the symmetric simple CSR.  A lock-free union-find over the E'
 * edges (the larger root hooked under the smaller by compare-and-swap: a find walks strictly decreasing ids, no thread waits for another) makes the
 * smallest vertex of every component its root.  One level-synchronous top-down BFS from all roots at once -- rows by length: <= VGL_BICC_SHORT (32) 8
 * lanes per row, <= VGL_BICC_WAVE (1024) a wavefront, longer a workgroup; one host read per level -- records level, parent and the vertices in level
 * order.  Per level and without host reads: size[v] of the subtrees (deepest level first), pre[v] (top level first; a child takes pre[p] + 1 + what its
 * earlier siblings took: the sibling order is arbitrary, subtree(v) = [pre[v], pre[v] + size[v]) is all that is used), and low / high[v] = min / max of
 * pre over subtree(v) and the far ends of its non-tree entries (a row pass with one writer per row, then integer atomicMin / atomicMax up the levels).
 * Per edge: a tree edge (child c, parent p) is a bridge iff low[c] >= pre[c] and high[c] < pre[c] + size[c]; if p is no root and low[c] < pre[p] or
 * high[c] >= pre[p] + size[p], the tree edges of c and p are united; a non-tree edge (a, b) unites the tree edges of a and b (in a BFS forest it never
 * joins a vertex to its ancestor).  The classes of that union-find over the tree edges (named by their child) are the blocks: the block of a tree
 * edge is that of its child, the block of a non-tree edge that of either end; the label is an atomicMin of the edge ids per class.  A cut vertex is a
 * row whose entries' edges carry two different labels.  A third union-find over the tree edges that are no bridges gives the 2-edge-connected
 * components; its roots are the smallest ids.  Work is O(V + E') in O(depth) launches; no cooperative launch, no grid barrier, no wait on a flag.
 * stats, all exact and the same on every run:
 *   undirected_edges = E'; components = connected components, isolated vertices included; bridges; articulation_points; biconnected_components;
 *   two_edge_components (= components + bridges); largest_component_edges = edges of the largest block (0 when E' = 0);
 *   depth = 1 + the largest BFS level, levels counted from the smallest vertex id of every component (0 when V = 0); prepared_now = this call built the
 *   edge numbering (stage 2 of the handle's cache).  articulation_points, biconnected_components and largest_component_edges are -1 when neither
 *   d_edge_component nor d_articulation was asked for: the block pass is then skipped.
 *   algorithmic_bytes, with nnz = 2 E' the entries of the symmetric CSR:
 *     92 V + 16 nnz + 24 E' + 104 (depth + 1)
 *       (V: degree read, union-find, level, size and cursor initialised 20; the root test 4; per BFS vertex its list entry written and read, its row
 *        bounds, level and parent written 24; pre: list entry, parent, size read, pre written 16; the local pass: list entry, row bounds, parent, pre
 *        read, low and high written 28.  nnz: the BFS and the local pass each read the entry and one word of its far end.  E': the endpoints read by the
 *        roots' union-find 8, endpoints and both parents read per edge 16.  depth: the 13 counters published per level and once after the seed.)
 *     + 16 E' with d_edge_u / d_edge_v (the endpoint arrays copied)  + E' with d_bridge
 *     + 33 V + 20 E' + 8 nnz when the block pass runs (V: the block union-find initialised and flattened 12, the smallest edge and the edge count per
 *        class initialised 8, the counts read 4, row bounds read and the flag written 9; E': the naming vertex written, read and replaced by the root,
 *        read and replaced by the label 20; nnz: the edge id of the slot and its label)
 *     + 12 V with d_two_edge_component (its union-find initialised, read and the label written).
 *     The size and low / high passes up the levels, the union-finds' walks, pre / low / high / size read per tree edge and the atomics' traffic are
 *     left out: a lower bound.  0 when V = 0.
 * Fails, before anything is written: a sharded handle, all six output pointers NULL, one of d_edge_u / d_edge_v without the other, E' >= 2^31 (from
 * the cache stage, as k-truss). */
typedef struct {
    int32_t depth;                      /* 1 + the largest BFS level from the smallest vertex of every component */
    int32_t prepared_now;               /* this call built the edge numbering */
    int64_t undirected_edges;           /* E' */
    int64_t components;                 /* connected components, isolated vertices included */
    int64_t bridges;
    int64_t articulation_points;        /* -1 when the block pass was skipped */
    int64_t biconnected_components;     /* -1 when the block pass was skipped */
    int64_t two_edge_components;
    int64_t largest_component_edges;    /* edges of the largest block; -1 when the block pass was skipped */
    int64_t algorithmic_bytes;
} vgl_hip_bicc_stats;
int vgl_hip_bicc_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int64_t *undirected_edges);
int vgl_hip_bicc_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_edge_u, int32_t *d_edge_v, uint8_t *d_bridge, int32_t *d_edge_component,
                     uint8_t *d_articulation, int32_t *d_two_edge_component, vgl_hip_bicc_stats *stats);

/* Maximal independent set (`mis`) and maximal matching (`matching`): the LEXICOGRAPHICALLY FIRST one under a fixed priority order, which is what the
 * sequential greedy algorithm returns when it takes the vertices (edges) in ascending order.  The reference has neither, so this comment is the contract:
 *   input     any handle that owns all rows; only the stored outgoing CSR is read.
 *   graph     the simple undirected graph of triangle counting's contract: u ~ v iff u != v and at least one of (u, v), (v, u) is stored.
 *   key       key(i, seed) = fmix32(i ^ fmix32(seed + 0x9e3779b9)), all in uint32 arithmetic; fmix32 is the murmur3 finaliser
 *             (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16), a bijection of uint32: default keys never tie.
 *   order     ascending (key, id), the smaller first; an equal key of a caller's array goes to the smaller id IN THE GRAPH'S OWN NUMBERING.
 *   The answer is unique, an integer, and does not depend on any VGL_MIS_* switch, on the order of the entries in a row or on the order in which the
 *   stores land (Blelloch, Fineman, Shun, SPAA 2012: the synchronous rounds below compute the greedy set).
 * vgl_hip_mis_run:  d_priority (uint32, V, device) or NULL = key(v, seed).  Outputs, either may be NULL but not both:
 *   d_in_set  uint8, V: 1 iff v is in the greedy set under the order;
 *   d_round   int32, V: +r if v entered the set in round r, -r if it was excluded in round r (never 0), under these SYNCHRONOUS rounds: in round r an
 *             undecided v goes OUT if a neighbour before it in the order is IN since a round < r; it goes IN if every neighbour before it is OUT since
 *             a round < r (an isolated vertex is IN in round 1); otherwise it stays undecided.  In closed form: round(IN v) = 1 + max |round(w)| over
 *             the neighbours w before v (1 if there are none); round(OUT v) = 1 + min round(w) over the IN neighbours w before v.
 *   Method: one int32 array holds the signed round (d_round itself when given); a reader treats |state| == r as undecided, so there is no double buffer
 *   and a store of the same launch is harmless.  The undecided rows are kept per row class of the symmetric simple CSR (<= VGL_MIS_SHORT (32): 8 lanes
 *   per row, <= VGL_MIS_WAVE (1024): a wavefront that stops at the first IN neighbour before v, longer: a workgroup); the key of an entry is computed
 *   (or gathered) first and the state read only for the entries before v.  One host read of the pinned mirror per round.  vgl_hip_mis_prepare (or the
 *   first run) builds stage 1 of the handle's cache, the symmetric simple CSR shared with kcore, ktruss, msf and bicc.
 *   timing slots: mis_init, mis_short, mis_wave, mis_wg, mis_publish, mis_finish.
 *   stats, all exact and the same on every run: rounds (0 when V = 0); set_size; prepared_now = this call built the symmetric CSR;
 *   live_total = the sum over the rounds of the number of undecided vertices at the start of the round (round 1: V);
 *   entries_walked = the sum over the rounds of the FULL row lengths of those vertices (an upper bound of what the early exit reads, exact by definition);
 *   algorithmic_bytes = 12 V (degree read, state cleared, list entry written) + 24 live_total (list entry read, row bounds read, state or list entry
 *   written) + 8 entries_walked (the adjacency entry and the state of its far end; a caller's priority array is left out) + 64 (rounds + 1) (the 8
 *   counters published after the classes are counted and after every round) + 5 V with d_in_set (state read, flag written): a lower bound; 0 when V = 0.
 * vgl_hip_matching_run:  edges carry the library's edge numbering of vgl_hip_ktruss_run (ascending (lo, hi) in the graph's own vertex numbering,
 *   E' < 2^31; stage 2 of the handle's cache, shared with ktruss, msf and bicc; vgl_hip_matching_prepare or the first run builds it and
 *   *undirected_edges (host, may be NULL) receives E').  d_edge_priority (uint32, E', device) or NULL = key(edge id, seed).  Outputs, each may be NULL
 *   but at least one must be given (the edge arrays are sized by the caller like k-truss's: E' <= stored entries):
 *   d_edge_u / d_edge_v  int32, E', both or neither: lo, hi of edge i;
 *   d_in_matching        uint8, E': 1 iff the edge is in the greedy matching over the edges ascending by (key, edge id);
 *   d_mate               int32, V: the partner of v, or -1;
 *   d_round              int32, V: the round in which v was matched, or 0.
 *   Rounds, two passes each.  Pass 1: every live vertex v takes best[v] = the minimum over its entries whose far end is unmatched of
 *   (key(e) << 32 | e); a vertex with no such entry leaves the worklist for good.  Pass 2: edge e = (u, v) is matched iff best[u] == best[v] == e;
 *   both ends write their mate, the lower end writes d_in_matching[e]; the unmatched vertices that have a best are live in the next round.  In round 1
 *   every vertex is live.  Method: pass 1 runs per row class (as above; the minimum is a 64-bit shuffle reduce per row group, the default key of an
 *   entry is computed, not gathered) and lists the vertices with a best; pass 2 is one launch over that list, whose length it reads from the device.
 *   timing slots: mm_init, mm_best_short, mm_best_wave, mm_best_wg, mm_match, mm_publish.
 *   stats, all exact and the same on every run: rounds (0 when V = 0); matched_edges; matched_vertices = 2 matched_edges; undirected_edges = E';
 *   prepared_now = this call built the edge numbering; live_total = the sum over the rounds of the live vertices of pass 1; entries_walked = the sum
 *   over the rounds of their full row lengths (pass 1 only);
 *   algorithmic_bytes = 20 V (degree read, mate and best initialised, list entry written) + 28 live_total (list entry read, row bounds read, best
 *   written) + 12 entries_walked (the adjacency entry, its edge id, the mate of its far end; a caller's priority array is left out) + 72 (rounds + 1)
 *   (the 9 counters published) + 16 E' with d_edge_u / d_edge_v (copied) + E' with d_in_matching (cleared) + 4 V with d_round (cleared); pass 2 is left
 *   out: a lower bound; 0 when V = 0.
 * Both fail, before anything is written: a sharded handle, all outputs NULL, one of d_edge_u / d_edge_v without the other, E' >= 2^31 (from the cache
 * stage, as k-truss).  V == 0 succeeds with rounds = 0 and writes nothing (vgl_hip_graph_create hands out no such handle: the smallest graph is one vertex
 * without an edge, rounds = 1). */
typedef struct {
    int32_t rounds;             /* synchronous rounds until every vertex is decided */
    int32_t prepared_now;       /* this call built the symmetric simple CSR */
    int64_t set_size;
    int64_t live_total;         /* sum over rounds of undecided vertices */
    int64_t entries_walked;     /* sum over rounds of their full row lengths */
    int64_t algorithmic_bytes;
} vgl_hip_mis_stats;
int vgl_hip_mis_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g);
int vgl_hip_mis_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const uint32_t *d_priority, uint32_t seed, uint8_t *d_in_set, int32_t *d_round,
                    vgl_hip_mis_stats *stats);
typedef struct {
    int32_t rounds;             /* two-pass rounds until no vertex is live */
    int32_t prepared_now;       /* this call built the edge numbering */
    int64_t matched_edges;
    int64_t matched_vertices;   /* 2 matched_edges */
    int64_t undirected_edges;   /* E' */
    int64_t live_total;         /* sum over rounds of live vertices */
    int64_t entries_walked;     /* sum over rounds of their full row lengths, first pass */
    int64_t algorithmic_bytes;
} vgl_hip_matching_stats;
int vgl_hip_matching_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int64_t *undirected_edges);
int vgl_hip_matching_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const uint32_t *d_edge_priority, uint32_t seed, int32_t *d_edge_u, int32_t *d_edge_v,
                         uint8_t *d_in_matching, int32_t *d_mate, int32_t *d_round, vgl_hip_matching_stats *stats);

/* Vertex similarity and link prediction (`sim`): the common neighbours of vertex pairs, and for a query vertex the k most similar vertices of its 2-hop
 * neighbourhood.  The reference has no such algorithm, so this comment is the contract:
 *   input     any handle that owns all rows; only the stored outgoing CSR is read.
 *   graph     the simple undirected graph of triangle counting's contract: u ~ v iff u != v and at least one of (u, v), (v, u) is stored.
 *   notation  N(u) = the neighbours of u (u is never in N(u)); d(u) = |N(u)|; c(u, v) = |N(u) & N(v)|; work2(u) = the sum of d(v) over v in N(u), the
 *             number of 2-paths that leave u.
 * vgl_hip_sim_prepare builds what is missing and nothing else: stage 1 of the handle's cache (the symmetric simple CSR, shared with kcore, ktruss, msf,
 *   bicc and mis) and work2 (int64, V; one pass, kept on the handle and freed with it).  Every entry below does the same on its first call.
 * vgl_hip_sim_pairs:  d_u / d_v (int32, n, device): n pairs in the graph's own numbering, in any order, repeated or not; u == v is allowed, c = d(u).
 *   d_common    int32, n: d_common[i] = c(u_i, v_i);
 *   d_weighted  float64, n: the sum of d_weight[w] over w in N(u_i) & N(v_i); needs d_weight (float64, V, device: finite values >= 0);
 *   d_degree    int32, V, optional: d(v), a copy of the cache's degrees (the rule of vgl_hip_tri_run).
 *   At least one of d_common / d_weighted must be given.  Jaccard c / (d(u) + d(v) - c), overlap c / min(d(u), d(v)), Sorensen 2 c / (d(u) + d(v)), the
 *   Adamic-Adar weights 1 / ln d(w), the resource-allocation weights 1 / d(w) and every other normalisation are the caller's business, in float64 (the
 *   rule of tri's clustering coefficient and msbfs's closeness).
 *   Method: the pairs are classified by the length of their SHORTER row (<= VGL_SIM_SHORT (32): 8 lanes per pair, <= VGL_SIM_WAVE (1024): a wavefront,
 *   longer: a workgroup) into one list per class (one counting pass that also validates, one appending pass; at most VGL_SIM_PAIR_CHUNK (2^28) pairs
 *   per list build); the lanes stride over the shorter row (u's when both are equally long) and binary-search the longer one.  Every pair has one
 *   owner: no atomic touches an output, and the outputs are written in the pairs' input order.
 *   Floating point: no floating-point atomics; every d_weighted[i] has one writer; lane l of L (8, 64, 256) adds the weights of its hits among the
 *   entries l, l + L, l + 2 L, ... of the shorter row in that order, starting from 0; the L partial sums are folded by the xor-shuffle tree (offsets
 *   L / 2, ..., 1 inside a wavefront; a workgroup adds its four wavefronts' sums in wavefront order).  The shape depends on the pair and the class
 *   bounds alone: the value is bit-identical from run to run under the same switches.  The library is built with -ffp-contract=off, without fast-math.
 *   timing slots: sim_work2, sim_classify, sim_publish, sim_pairs_short, sim_pairs_wave, sim_pairs_wg.
 *   stats, all exact and the same on every run: pairs = n; pairs_short / pairs_wave / pairs_wg; elements_examined = the sum of min(d(u), d(v)) over the
 *   pairs; common_total = the sum of c; prepared_now = this call built work2;
 *   algorithmic_bytes = 64 n (per pair: u, v and both degrees read by the counting pass 16, the list entry written and read 8, u, v read again 8, the
 *   bounds of both rows 32) + 4 elements_examined (the entries of the shorter rows; the searches in the longer rows are left out) + 4 n with d_common
 *   + 8 n + 8 common_total + 8 V with d_weighted (the sum written, the weights of the hits gathered, the weights validated) + 8 V with d_degree
 *   (copied): a lower bound.
 *   Fails, before anything is written: a NULL ctx or graph, a sharded handle, n < 0, a vertex outside [0, V) (found by the counting pass), d_weighted
 *   without d_weight, a NaN, infinite or negative weight (one pass over V), both outputs NULL.  n == 0 succeeds and writes nothing but d_degree.
 * vgl_hip_sim_topk:  d_queries (int32, n, device): vertex ids, repeats allowed, each a row of its own; NULL = all V vertices in id order (n must equal V).
 *   The candidates of a query u are the vertices w != u with c(u, w) >= 1; unless include_neighbours is 1 the members of N(u) are excluded (link
 *   prediction).  metric, the score of a candidate:
 *     VGL_HIP_SIM_COMMON   c;   VGL_HIP_SIM_JACCARD  c / (d(u) + d(w) - c);   VGL_HIP_SIM_OVERLAP  c / min(d(u), d(w)).
 *   Sorensen 2 c / (d(u) + d(w)) = 2 J / (1 + J) is monotone in the Jaccard score J and so ranks exactly as Jaccard: it has no code of its own.
 *   Scores are compared AS FRACTIONS in int64: a beats b iff num_a den_b > num_b den_a (no overflow: num, den < 2^31).  Equal scores go to the smaller
 *   d_label[w] (int32, V, device, distinct; NULL = the vertex id itself; a caller that renumbered the graph passes the original ids, so the answer does
 *   not depend on the numbering).  The order is strict and total: the output is unique.
 *   d_ids / d_common  int32, n x k, row-major, indexed with int64: row i holds the best min(k, candidates) candidates of query i, best first, in the
 *   graph's own numbering, and their c; the remaining slots hold -1 and 0.  d_common may be NULL.  1 <= k <= VGL_HIP_SIM_MAX_K.
 *   Method: one workgroup per query, classified by work2(u), the upper bound of its distinct candidates: <= VGL_SIM_TABLE_SMALL (1024) an LDS
 *   open-addressing table of 2048 (id, count) slots; <= VGL_SIM_TABLE (8192) one of 16384 slots (128 KiB: one workgroup per CU, which is why there are
 *   two table classes); beyond, a dense int32 counter array of V entries and a touched list of V entries in a scratch slot.  A scratch slot belongs to
 *   one resident workgroup; there are min(VGL_SIM_SCRATCH_MB (4096) MiB / 8 V bytes, global rows, 1024) of them, at least 1.  The row is expanded by
 *   walking N(v) for every v in N(u) and counting w; a counter whose atomic add returns 0 appends w to the touched list, which is what gets scored
 *   and what clears the counters for the slot's next row.  u and (by default) N(u) are struck out after the count.  Selection, the same in all
 *   classes: k rounds of a workgroup arg-max over the candidates that come strictly after the previous pick in the order above: stateless and exact,
 *   k x candidates comparisons.
 *   timing slots: sim_work2, sim_classify, sim_publish, sim_topk_small, sim_topk_table, sim_topk_global.
 *   stats, all exact and the same on every run: queries = n; rows_small / rows_table / rows_global; two_paths_walked = the sum of work2 over the
 *   queries; candidates_total = the distinct candidates summed over the queries, after the exclusion; filled = the output slots that hold a vertex;
 *   scratch_slots (0 when no row is global); prepared_now = this call built work2;
 *   algorithmic_bytes = 36 n (per query: its id and work2 read by the counting pass 12, the list entry written and read 8, its row bounds 16)
 *   + 4 two_paths_walked (the entries of the neighbours' rows) + 4 n k (d_ids) + 4 n k with d_common; the query's own row, the neighbours' row bounds,
 *   the counters, the touched lists and the k selection rounds are left out: a lower bound.
 *   Fails, before anything is written: a NULL ctx or graph, a sharded handle, k out of range, an unknown metric, a query outside [0, V), n < 0,
 *   d_queries == NULL with n != V, d_ids == NULL.  n == 0 succeeds and writes nothing.
 * No output depends on any VGL_SIM_* switch except the last bits of d_weighted, whose summation shape follows the class bounds. */
#define VGL_HIP_SIM_COMMON 0
#define VGL_HIP_SIM_JACCARD 1
#define VGL_HIP_SIM_OVERLAP 2
#define VGL_HIP_SIM_MAX_K 64
typedef struct {
    int64_t pairs;
    int64_t pairs_short;        /* pairs per class of the shorter row */
    int64_t pairs_wave;
    int64_t pairs_wg;
    int64_t elements_examined;  /* sum of min(d(u), d(v)) */
    int64_t common_total;       /* sum of c */
    int64_t algorithmic_bytes;
    int32_t prepared_now;       /* this call built work2 */
} vgl_hip_sim_pairs_stats;
typedef struct {
    int64_t queries;
    int64_t rows_small;         /* queries per class of work2 */
    int64_t rows_table;
    int64_t rows_global;
    int64_t two_paths_walked;   /* sum of work2 over the queries */
    int64_t candidates_total;   /* distinct candidates after the exclusion */
    int64_t filled;             /* output slots that hold a vertex */
    int64_t scratch_slots;      /* resident workgroups of the global class */
    int64_t algorithmic_bytes;
    int32_t prepared_now;       /* this call built work2 */
} vgl_hip_sim_topk_stats;
int vgl_hip_sim_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g);
int vgl_hip_sim_pairs(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_u, const int32_t *d_v, int64_t n, const double *d_weight, int32_t *d_common,
                      double *d_weighted, int32_t *d_degree, vgl_hip_sim_pairs_stats *stats);
int vgl_hip_sim_topk(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_queries, int32_t n, int metric, int32_t k, int include_neighbours,
                     const int32_t *d_label, int32_t *d_ids, int32_t *d_common, vgl_hip_sim_topk_stats *stats);

/* Subgraph extraction (`subgraph`), bounded multi-seed reach (`khop`) and fixed-fanout neighbour sampling (`sample`): the part of a graph that a mask,
 * a neighbourhood or a sample selects, handed back as CSR.  The reference has nothing of the kind, so this comment is the contract:
 *   input     any handle that owns all rows.  Every id is in the graph's own numbering.  Direction 0 is the stored outgoing CSR, direction 1 the stored
 *             incoming CSR; direction 1 on a handle without an incoming CSR is an error.  The stored entries are taken as they are: self-loops and
 *             repeated entries are entries like any other (this is NOT the simple graph of triangle counting's contract).
 * The stable row filter, vgl_hip_subgraph_plan_create / _info / _vertex_maps / _fill / _destroy:
 *   d_keep_vertex  uint8, V, device: nonzero = keep the vertex; NULL = keep all.
 *   d_keep_entry   uint8, one per stored OUTGOING entry in CSR order (as sssp takes weights), device: nonzero = keep; NULL = keep all.  Borrowed until
 *                  the last fill of the plan.  At least one of the two masks must be given.
 *   new_id[v] (int32, V) = the number of kept vertices below v for a kept v, -1 for a dropped one; old_id (int32, V') is its inverse.  The relabelling is
 *   MONOTONE.  In direction d, row new_id[v] of the result holds exactly those entries of row v whose far end is kept and, in direction 0, whose entry
 *   flag is nonzero, relabelled, IN THEIR STORED ORDER.  d_origin (int64, optional) receives the position in the parent's adjacency array of that
 *   direction of every surviving entry: weights follow with vgl_hip_gather_u32.  With d_keep_entry only direction 0 can be filled (the flags are per
 *   outgoing entry); the caller builds the incoming CSR of such a result by the transposition Graph.from_coo uses.  With a vertex mask alone both
 *   directions are filled by the same kernels.  Because the relabelling is monotone and both filters are stable, the result is BIT-IDENTICAL, rowptr
 *   and adj of both directions, to what the stable COO -> CSR build (vgl_hip_coo_to_csr, then the same build over the transposed list taken in
 *   outgoing CSR order) makes of the filtered, relabelled edge list taken in the parent's outgoing CSR order -- provided the parent's incoming CSR was
 *   built that way too.
 *   Method: the plan validates, scans the vertex mask (tile sums, their scan, an apply pass), counts and lists the kept rows per class of their FULL
 *   length and per direction (<= VGL_SUB_SHORT (32): 8 lanes per row, <= VGL_SUB_WAVE (1024): a wavefront, longer: a workgroup), counts the survivors
 *   of every kept row with one kernel per class, and scans the counts into the new int64 rowptr.  The host reads the pinned counter mirror twice (the
 *   list sizes; V', E'out, E'in) and the plan synchronises the stream once, at its end.  _info hands V', E'out, E'in (-1 when direction 1 cannot be
 *   filled) and the stats to the host; _vertex_maps copies new_id / old_id (either may be NULL); _fill(direction) copies the plan's rowptr into d_rowptr
 *   (int64, V' + 1) and writes d_adj (int32, E') and d_origin (int64, E', optional) -- buffers of the caller, which a handle made of them borrows as
 *   vgl_hip_graph_create always does -- and is left enqueued on the context's stream.  The fill is an ORDERED compaction: every row has one owner, a
 *   survivor's position is the row's new start + the survivors of the chunks before (a running base) + the survivors before it in its chunk (ballot
 *   and popcount of the lanes below within the 8-lane group or the wavefront; across the four wavefronts of a workgroup an LDS scan).  No atomic
 *   touches an output.  V' == 0 is a valid plan; its fill writes nothing.
 *   timing slots: sub_scan (scans, classification, lists), sub_count_short / _wave / _wg, sub_publish, sub_fill_short / _wave / _wg.
 *   stats, all exact and the same on every run: vertices_kept = V'; rows_{short,wave,wg}_{out,in} = kept rows per class of their full length (the only
 *   stats that follow VGL_SUB_SHORT / VGL_SUB_WAVE); entries_read_{out,in} = the sum of the full lengths of the kept rows; entries_kept_{out,in} = E' of
 *   the direction; the _in fields are 0 when direction 1 is not planned;
 *   algorithmic_bytes = V with d_keep_vertex (the mask read) + 4 V (new_id written) + 4 V' (old_id written) + for every planned direction
 *   56 V' (counting and filling each: list entry 4, row bounds 16, count written or new row start read 8) + 32 (V' + 1) (the counts scanned: read and
 *   written; the rowptr copied out: read and written) + 16 read (counting and filling each: the adjacency entry and the new id of its far end)
 *   + 2 read with d_keep_entry (the flag, twice) + 4 kept (the new adjacency written); the classification pass over V and d_origin are left out: a lower
 *   bound of a plan followed by one fill per planned direction.
 *   Fails, before anything is written: a NULL ctx, graph or out pointer, a sharded handle, both masks NULL; _fill: a direction other than 0 / 1,
 *   direction 1 on a plan with an entry mask or without an incoming CSR, a NULL d_rowptr (or d_adj while E' > 0) unless V' == 0.
 * vgl_hip_khop_run:  d_seeds (int32, n, device; repeats allowed; n == 0 succeeds with every d_hop = -1), hops >= 0, direction, symmetric (nonzero: follow
 *   the stored entries of BOTH directions; needs the incoming CSR, direction is then ignored).
 *   d_hop[v] (int32, V, device) = the smallest number of steps from any seed to v if that is <= hops, else -1; hops == 0 marks the seeds alone.  Direction 1
 *   steps along incoming entries (d_hop[v] = the steps from v to the nearest seed along stored edges).  An integer, unique.
 *   Method: the seeds are validated by one pass, d_hop is set to -1 and the seeds to 0, then level-synchronous top-down steps
 *   (vgl_hip_bfs_step_top_down and its frontier compaction) on the handle, on the handle with the two directions swapped (built on first use and kept
 *   on the handle, as scc does) or on both, until `hops` levels were expanded or a level is empty.
 *   timing slots: khop_init, khop_publish, khop_count and those of the top-down step.
 *   stats, all exact: reached = the entries of d_hop that are >= 0; levels_run = the non-empty levels that were expanded (at most hops);
 *   frontier_total = the sum of their sizes; edges_examined = the sum of the full row lengths of their vertices in every followed direction.
 *   Fails, before anything is written: a NULL ctx, graph or d_hop, a sharded handle, n < 0, hops < 0, a seed outside [0, V), a direction other than
 *   0 / 1, direction 1 or symmetric without the incoming CSR.
 * vgl_hip_sample_neighbors:  d_seeds (int32, n, device; repeats allowed, each a row of its own), fanout >= 1, direction, seed (uint32).
 *   Row i of the output holds the min(fanout, degree) entries of the row of d_seeds[i] with the smallest key(p mod 2^32, seed), p = the entry's
 *   position in the adjacency array of that direction; key is mis's key(i, seed) above.  fmix32 is a bijection, so the keys of an array of fewer than
 *   2^32 entries never tie; a longer array is refused.  The chosen entries are written IN ASCENDING POSITION.  The answer is unique and depends on
 *   no switch; it DOES depend on the graph's numbering (the positions are those of this handle's arrays).  Sampling is without replacement over the
 *   stored entries: a repeated entry can be drawn once per copy.
 *   d_rowptr (int64, n + 1; d_rowptr[n] = the total), d_adj (int32, capacity n * fanout, indexed with int64), d_origin (int64, same capacity, optional:
 *   the positions p).
 *   Method: the key is a function of the position alone, so the selection reads no memory; only the emit gathers adj[p].  One pass validates the seeds
 *   and writes min(fanout, degree) per seed, a scan makes d_rowptr, the seeds are listed per class of their degree (<= VGL_SAMPLE_SHORT (32): 8 lanes,
 *   <= VGL_SAMPLE_WAVE (1024): a wavefront, longer: a workgroup).  A row of at most fanout entries is copied.  Short and wave rows rank-count: an entry
 *   is taken when fewer than fanout entries of its row have a smaller key (degree^2 / lanes key evaluations per lane at most).  Workgroup rows find the
 *   fanout-th smallest key by a 4 x 8-bit radix select over recomputed keys (LDS histograms, 5 passes over the positions in all).  The emit is the
 *   ordered compaction of the filter above.
 *   timing slots: sample_count (validation, scan, lists), sample_publish, sample_short, sample_wave, sample_wg.
 *   stats, all exact and the same on every run: seeds = n; rows_short / rows_wave / rows_wg (the only stats that follow the two switches);
 *   entries_examined = the sum of the seeds' degrees; sampled_total = d_rowptr[n];
 *   algorithmic_bytes = 60 n (per seed: its id and row bounds read and the count written 28, the list entry, the id, the row bounds and the new row
 *   start read 32) + 16 (n + 1) (the counts scanned) + 8 sampled_total (adj[p] read, d_adj written); the list build and d_origin are left out: a lower bound.
 *   Fails, before anything is written: a NULL ctx, graph, d_rowptr (or d_adj while n > 0), a sharded handle, n < 0 or n >= 2^31, fanout < 1, a seed
 *   outside [0, V), a direction other than 0 / 1, direction 1 without the incoming CSR, an adjacency array of 2^32 entries or more.
 * No output depends on VGL_SUB_* or VGL_SAMPLE_*. */
typedef struct vgl_hip_subgraph_plan vgl_hip_subgraph_plan;
typedef struct {
    int64_t vertices_kept;      /* V' */
    int64_t rows_short_out;     /* kept rows per class of their full length, outgoing */
    int64_t rows_wave_out;
    int64_t rows_wg_out;
    int64_t rows_short_in;      /* ... incoming (0 when direction 1 is not planned) */
    int64_t rows_wave_in;
    int64_t rows_wg_in;
    int64_t entries_read_out;   /* sum of the full lengths of the kept rows */
    int64_t entries_read_in;
    int64_t entries_kept_out;   /* E' of the direction */
    int64_t entries_kept_in;
    int64_t algorithmic_bytes;
} vgl_hip_subgraph_stats;
int vgl_hip_subgraph_plan_create(vgl_hip_ctx *ctx, vgl_hip_graph *g, const uint8_t *d_keep_vertex, const uint8_t *d_keep_entry,
                                 vgl_hip_subgraph_plan **out);
int vgl_hip_subgraph_plan_info(vgl_hip_subgraph_plan *plan, int32_t *vertices, int64_t *out_entries, int64_t *in_entries, vgl_hip_subgraph_stats *stats);
int vgl_hip_subgraph_plan_vertex_maps(vgl_hip_ctx *ctx, vgl_hip_subgraph_plan *plan, int32_t *d_new_id, int32_t *d_old_id);
int vgl_hip_subgraph_plan_fill(vgl_hip_ctx *ctx, vgl_hip_subgraph_plan *plan, int direction, int64_t *d_rowptr, int32_t *d_adj, int64_t *d_origin);
int vgl_hip_subgraph_plan_destroy(vgl_hip_ctx *ctx, vgl_hip_subgraph_plan *plan);
typedef struct {
    int64_t reached;            /* entries of d_hop that are >= 0 */
    int64_t frontier_total;     /* sum of the sizes of the expanded levels */
    int64_t edges_examined;     /* sum of their full row lengths, every followed direction */
    int32_t levels_run;         /* non-empty levels expanded */
} vgl_hip_khop_stats;
int vgl_hip_khop_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_seeds, int64_t n, int32_t hops, int direction, int symmetric, int32_t *d_hop,
                     vgl_hip_khop_stats *stats);
typedef struct {
    int64_t seeds;
    int64_t rows_short;         /* seeds per class of their degree */
    int64_t rows_wave;
    int64_t rows_wg;
    int64_t entries_examined;   /* sum of the seeds' degrees */
    int64_t sampled_total;      /* d_rowptr[n] */
    int64_t algorithmic_bytes;
} vgl_hip_sample_stats;
int vgl_hip_sample_neighbors(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_seeds, int64_t n, int32_t fanout, int direction, uint32_t seed,
                             int64_t *d_rowptr, int32_t *d_adj, int64_t *d_origin, vgl_hip_sample_stats *stats);

/* The quotient graph of a vertex labelling (`quotient`): the vertices of a class merge into one coarse vertex, the stored entries between two classes
 * into one coarse entry that carries their summed weight.  The row MERGE next to the row filter above; the condensation of the SCC labels, the
 * coarsening step of a multilevel method, the numbers behind modularity.  The reference has nothing of the kind, so this comment is the contract:
 *   input     any handle that owns all rows.  d_label: int32, V entries, device, in the graph's own numbering; every value >= 0; the values are opaque.
 *             The stored entries are taken as they are: self-loops and repeated entries are entries like any other (as for the row filter; this is
 *             NOT the simple graph of triangle counting's contract).
 *   coarse vertices   V' = the number of distinct label values; c(v) = the rank of d_label[v] among the distinct values in ascending order, so the
 *             numbering is a function of the label values alone, independent of the graph's vertex numbering.  cluster_of[v] = c(v) (int32, V);
 *             label_of[c] (int32, V', ascending); size[c] (int32, V'); members (int32, V: the vertices grouped by cluster, ascending id within a
 *             cluster) and member_ptr (int64, V' + 1).
 *   coarse entries in direction d (0 = the stored outgoing CSR, 1 = the stored incoming CSR; direction 1 on a handle without one is an error):
 *             row c holds one entry per distinct c(w) over the stored entries (v, w) of that direction with c(v) = c, ASCENDING and free of repeats;
 *             with drop_loops nonzero the entries with c(v) == c(w) are left out.  d_count[i] (int64, E') = the sum over the merged stored entries p
 *             of d_weight[p] (int64, optional, one per stored entry of THAT direction in CSR order; NULL = 1 each: the multiplicity).  Sums are
 *             two's-complement int64; the caller keeps the totals below 2^63 (not checked).  Integer addition is associative, so the answer is unique
 *             and depends on no switch, launch order or atomic order.  Because every row ascends, the result is BIT-IDENTICAL, rowptr and adj of both
 *             directions, to Graph.from_coo (the stable COO -> CSR build) on the ascending list of the distinct coarse pairs.
 *   vgl_hip_quotient_plan_create / _info / _vertex_maps / _members / _fill / _destroy, after vgl_hip_subgraph_plan_*:  _info hands V', E'out, E'in (-1
 *             without an incoming CSR) and the stats to the host; _vertex_maps copies cluster_of / label_of / size, _members copies members /
 *             member_ptr (every pointer optional); _fill(direction, d_weight) copies the plan's rowptr into d_rowptr (int64, V' + 1) and writes d_adj
 *             (int32, E') and d_count (int64, E') -- buffers of the caller -- and is left enqueued on the context's stream.  A coarse row without
 *             entries is valid (the last row, a cluster whose members are all isolated).
 *   Method, vertex side: one validation pass (negative labels, the largest label); rocprim::radix_sort_pairs on (label, vertex) over the bits the
 *             largest label needs (stable: the sorted vertices are `members`); head flags, their inclusive scan and a scatter give cluster_of,
 *             label_of, member_ptr and size.  Per planned direction member_off = the exclusive scan of the members' row lengths in member order: flat
 *             entry j of coarse row c finds its member by a binary search of member_off within the cluster (a cluster of many short rows costs no
 *             trip per member); the row's VOLUME (the stored entries of its members) is a difference of two member_off values.
 *   Method, entry side: coarse rows are classified by volume and listed per class (rows of volume 0 are no items):
 *             <= VGL_QUOT_SHORT (32; at most 256): 8 lanes per row, rank-counting over the gathered coarse far ends, 8 at a time in registers and
 *               exchanged by shuffles: an entry is a head when no equal key sits at an earlier flat position, its output position is the number of
 *               heads with a smaller key, its count the sum over the equal keys;
 *             <= VGL_QUOT_WAVE (1024; at most 1024): a wavefront per row;  <= VGL_QUOT_TABLE (4096; at most 4096): a workgroup per row: the coarse
 *               far ends are gathered through cluster_of into LDS and sorted there (bitonic), the distinct keys are compacted in place with the
 *               team's rank, and the fill adds every entry's weight to the LDS int64 sum of its key (binary search, LDS atomic add), then writes
 *               keys and sums in order.  A row at the bound always fits: the LDS arrays hold one key and one sum per ENTRY;
 *             larger: keys  c << 32 | c(w)  paired with the weight, rocprim::radix_sort_pairs then rocprim::reduce_by_key, in pieces of consecutive
 *               rows whose buffers (32 bytes per key) stay under VGL_QUOT_SORT_CAP_MB (4096; 0 = no cap; a row above the cap is a piece of its own);
 *               the runs of row c are placed at the row's start.
 *             A count pass (the kernels with FILL = false) gives the distinct entries per row, a scan the int64 rowptr; the fill pass (FILL = true)
 *             writes adj and count.  Every row has one owner; no atomic touches an output array; no floating point, no cooperative launch, no wait
 *             on a flag.  The host reads the pinned counter mirror FOUR times per plan (the label check; V'; the class sizes of both directions; E'
 *             of both directions) and copies the volumes of the sorted rows once per direction that has any (to cut the pieces).
 *   timing slots: quot_check, quot_vertex (sort, heads, scan, scatter, sizes), quot_member_off, quot_classify, quot_lists, quot_count_short / _wave /
 *             _table / _sorted, quot_scan, quot_publish, quot_fill_short / _wave / _table / _sorted (one _sorted bracket per piece).
 *   stats, all exact and the same on every run: vertices = V'; rows_{short,wave,table,sorted}_{out,in} = coarse rows of volume > 0 per class;
 *             entries_read_{out,in} = the stored entries of the direction; entries_{out,in} = E'; sorted_keys_{out,in} = the volumes of the sorted
 *             rows; sort_pieces_{out,in}.  Only rows_*, sorted_keys_* and sort_pieces_* follow the switches; the _in fields are 0 when direction 1 is
 *             not planned.
 *             algorithmic_bytes = 32 V (labels read by the check 4; label and vertex read and written once by the sort 16, a lower bound of its
 *             passes; cluster_of written 4; members read by the scatter 4; head and rank of the position 4) + 8 V' (label_of, size) + 8 (V' + 1)
 *             (member_ptr) + for every planned direction 28 V (member_off: the member 4, its row bounds 16, the offset written 8) + 40 (V' + 1)
 *             (the counts written 8, scanned: read 8 and written 8; the rowptr copied out: read 8 and written 8) + 16 read (counting and filling each:
 *             the adjacency entry 4 and the cluster of its far end 4) + 12 E' (adj 4 and count 8 written); the binary searches, the lists, the sort
 *             buffers and d_weight are left out: a lower bound of a plan followed by one fill per planned direction.
 *   Fails, before anything is written: a NULL ctx, graph, label or out pointer, a sharded handle, a negative label; _fill: a direction other than
 *             0 / 1, direction 1 without the incoming CSR, a NULL d_rowptr, a NULL d_adj or d_count while E' > 0.
 * No output depends on VGL_QUOT_*. */
typedef struct vgl_hip_quotient_plan vgl_hip_quotient_plan;
typedef struct {
    int64_t vertices;           /* V' */
    int64_t rows_short_out;     /* coarse rows of volume > 0 per class, outgoing */
    int64_t rows_wave_out;
    int64_t rows_table_out;
    int64_t rows_sorted_out;
    int64_t rows_short_in;      /* ... incoming (0 when direction 1 is not planned) */
    int64_t rows_wave_in;
    int64_t rows_table_in;
    int64_t rows_sorted_in;
    int64_t entries_read_out;   /* the stored entries of the direction */
    int64_t entries_read_in;
    int64_t entries_out;        /* E' of the direction */
    int64_t entries_in;
    int64_t sorted_keys_out;    /* the volumes of the sorted rows */
    int64_t sorted_keys_in;
    int64_t sort_pieces_out;
    int64_t sort_pieces_in;
    int64_t algorithmic_bytes;
} vgl_hip_quotient_stats;
int vgl_hip_quotient_plan_create(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_label, int drop_loops, vgl_hip_quotient_plan **out);
int vgl_hip_quotient_plan_info(vgl_hip_quotient_plan *plan, int32_t *vertices, int64_t *out_entries, int64_t *in_entries, vgl_hip_quotient_stats *stats);
int vgl_hip_quotient_plan_vertex_maps(vgl_hip_ctx *ctx, vgl_hip_quotient_plan *plan, int32_t *d_cluster_of, int32_t *d_label_of, int32_t *d_size);
int vgl_hip_quotient_plan_members(vgl_hip_ctx *ctx, vgl_hip_quotient_plan *plan, int32_t *d_members, int64_t *d_member_ptr);
int vgl_hip_quotient_plan_fill(vgl_hip_ctx *ctx, vgl_hip_quotient_plan *plan, int direction, const int64_t *d_weight, int64_t *d_rowptr, int32_t *d_adj,
                               int64_t *d_count);
int vgl_hip_quotient_plan_destroy(vgl_hip_ctx *ctx, vgl_hip_quotient_plan *plan);

/* Louvain move rounds (`louvain`): one level of a search for a partition of high modularity by synchronous INTEGER move rounds.  The reference has
 * nothing of the kind, so this comment is the contract.  No floating point takes part in any decision; no result depends on an atomic or launch
 * order; every loop has a bound; every output is a function of the graph in its own numbering, the weights, seed, max_rounds and min_gain_den, and
 * of no switch.  Unlike mis the result is NOT invariant under renumbering: ties and the swap guard go by the graph's own ids.  Only the level is
 * here: the multi-level run (the quotient of a level's graph by its result as the next level's graph) is not part of the library yet.
 *   one level (vgl_hip_louvain_move, on any handle whose stored outgoing CSR the caller vouches is symmetric): the stored CSR as it is, repeats and
 *             loops allowed, int64 weights per stored entry (NULL = 1 each; negative or m >= 2^31 fails).  k_v = the weight of row v, loops
 *             included; m = sum k_v; a SELF ENTRY is an entry (v, v).  Start: comm[v] = v (a community is named by a vertex id);
 *             tot[c] = sum of k_v over the members, size[c] = their number.  Round r = 1, 2, ... <= max_rounds does, in order:
 *             1. every vertex is evaluated against the snapshot (comm, tot, size): k(v, C) = the weight of v's non-self entries whose far end is
 *                in C; the candidates are the communities of the non-self neighbours and A = comm[v] (k(v, A) may be 0);
 *                score(C) = k(v, C) m - k_v tot'(C) with tot'(A) = tot[A] - k_v and tot'(C) = tot[C] otherwise; best(v) = the candidate of greatest
 *                score, a tie to the smallest community id; v WANTS to move when best != A, score(best) > score(A) and not (size[A] == 1 and
 *                size[best] == 1 and best > A) -- the swap guard: of two singletons that would trade places only the larger id moves.
 *                W_r = the vertices that want to move; I_r = sum over v of k(v, A) + the weight of v's self entries;
 *                N_r = m I_r - sum over c of tot[c]^2, the exact modularity numerator: Q = N_r / m^2.
 *             2. if round r - 1 applied at least one move and N_r <= N_kept: the result is the kept assignment (the one before those moves),
 *                outcome REVERTED, stop.
 *             3. kept = comm, N_kept = N_r.  If min_gain_den D > 0, round r - 1 applied a move and N_r - N_{r-1} < floor(m^2 / D): outcome
 *                SMALL_GAIN, the result is comm, stop (D = 0 disables the test).
 *             4. W_r == 0: outcome CONVERGED, the result is comm, stop.
 *             5. r == max_rounds: outcome CAPPED, the result is comm (this round's moves are not applied), stop.
 *             6. comm[v] = best(v) for the vertices that want to move and are ACTIVE in round r: active(v, r) = key(v, seed + r) & 1 with mis's
 *                key(i, s) = fmix32(i ^ fmix32(s + 0x9e3779b9)), uint32 arithmetic.  All moves of a round read the same snapshot; tot and size are
 *                recounted.  A round may apply no move although W_r > 0; the next round is then not judged in step 2.
 *             N_kept strictly increases over the judged rounds, so a level ends and its result is never worse than the singletons.
 *             vgl_hip_louvain_move writes d_label (int32, V): the vertex that names v's community.  m == 0: every vertex is its own community,
 *             CONVERGED after one round, N = 0.
 *   Method    rows are classified once per level by length: <= VGL_LOUVAIN_SHORT (32) 8 lanes per row, rank-counting over the gathered comm[adj]
 *             in chunks of 8 exchanged by shuffles (a head has no equal key before it, k(v, C) at a head is the sum over the equal keys);
 *             <= VGL_LOUVAIN_WAVE (1024, at most 1024) a wavefront and <= VGL_LOUVAIN_WG (4096, at most 4096) a workgroup per row: keys staged in
 *             LDS, a bitonic sort, the distinct keys compacted with the team's rank, one LDS int64 sum per distinct key (binary search, LDS integer
 *             add), 12 bytes per entry; longer rows: keys  row << 32 | comm[w]  (a self entry's low half is 0xffffffff) paired with the weight,
 *             rocprim::radix_sort_pairs and rocprim::reduce_by_key in pieces of consecutive rows whose buffers (32 bytes per key) stay under
 *             VGL_LOUVAIN_SORT_CAP_MB (4096; 0 = no cap), then a wavefront per row scores the row's runs.  Every class picks with the team's
 *             reductions: the greatest score, then the smallest id among the equal scores.  I and W go to int64 counters, one atomic per wave.
 *             The apply is double-buffered (kept is the other buffer); the host reads the pinned counter mirror once per round (I, sum tot^2, W,
 *             applied) and twice more per level; the sort scratch is sized for the largest piece before the round loop (it grows there only if a smaller
 *             piece asks for more).
 *   timing slots: louvain_prepare, louvain_eval_short / _wave / _wg / _sorted (one _sorted bracket per piece), louvain_reduce, louvain_apply,
 *             louvain_publish (the counter mirror).
 *   stats, all exact and the same on every run (the struct has room for the levels of a run; the move fills level 0): levels = 1; prepared_now = 0;
 *             total_weight = m; modularity_num = N of the result; entries_walked = rounds x entries; rows_short / _wave / _wg / _sorted, sorted_keys, sort_pieces: the
 *             rows of length > 0 per class, the entries of the sorted rows and their pieces at level 0 (only these follow the switches);
 *             per level l < levels: vertices, entries, communities (of the result), rounds (evaluated), outcome, level_modularity_num = N_kept.
 *             algorithmic_bytes = sum over the levels of [ 8 (V_l + 1) (rowptr read for k) + (4 + wb) E_l (adj, weight) + 24 V_l (k 8, comm 4,
 *             tot 8, size 4 written) + rounds_l ((8 + wb) E_l (adj 4, the far end's comm 4, weight wb) + 44 V_l (row bounds 8, k 8, comm 4, tot 8,
 *             size 4, best written 4; tot read by the reduce 8)) + (rounds_l - 1) 32 V_l (the apply: best 4, comm read 4 and written 4, k 8, tot 8
 *             and size 4 recounted) ], wb = 8 where the level reads weights (iff d_weight) and 0 otherwise.
 *             Scratch, lists and sort buffers are left out: a lower bound.
 *   Fails, before anything is written: a NULL ctx, graph or output pointer, a sharded handle, max_rounds < 1 or > 65535, min_gain_den < 0, a
 *             negative weight, m >= 2^31. */
#define VGL_HIP_LOUVAIN_MAX_LEVELS 32
enum { VGL_HIP_LOUVAIN_CONVERGED = 0, VGL_HIP_LOUVAIN_REVERTED = 1, VGL_HIP_LOUVAIN_SMALL_GAIN = 2, VGL_HIP_LOUVAIN_CAPPED = 3 };
typedef struct {
    int32_t levels;
    int32_t prepared_now;       /* this call built the cache stage it needs */
    int64_t total_weight;       /* m */
    int64_t modularity_num;     /* N of the result: Q = N / m^2 */
    int64_t entries_walked;     /* sum over levels of rounds x entries */
    int64_t algorithmic_bytes;
    int64_t rows_short;         /* level 0: rows of length > 0 per class */
    int64_t rows_wave;
    int64_t rows_wg;
    int64_t rows_sorted;
    int64_t sorted_keys;        /* level 0: the entries of the sorted rows */
    int64_t sort_pieces;
    int64_t vertices[VGL_HIP_LOUVAIN_MAX_LEVELS];
    int64_t entries[VGL_HIP_LOUVAIN_MAX_LEVELS];
    int64_t communities[VGL_HIP_LOUVAIN_MAX_LEVELS];
    int64_t level_modularity_num[VGL_HIP_LOUVAIN_MAX_LEVELS];
    int32_t rounds[VGL_HIP_LOUVAIN_MAX_LEVELS];
    int32_t outcome[VGL_HIP_LOUVAIN_MAX_LEVELS];
} vgl_hip_louvain_stats;
int vgl_hip_louvain_move(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int64_t *d_weight, int32_t max_rounds, int64_t min_gain_den, uint32_t seed,
                         int32_t *d_label, vgl_hip_louvain_stats *stats);

/* Batched personalised PageRank (`ppr`): rank with restart at a seed set, for many seed sets per pass over the adjacency, float64, with the damping
 * and the stopping tolerance of the caller's choice; the empty seed list is plain PageRank as networkx and cuGraph define it.  vgl_hip_pr_run above is
 * the reference's benchmark kernel (float32, damping 0.85, a fixed iteration count, one vector) and stays as it is.  The reference has no
 * counterpart, so this comment is the contract:
 *   graph     the stored DIRECTED graph of a handle that owns all rows.  Every stored entry counts: a multi-edge with its multiplicity, a self entry
 *             as an edge like any other.  outdeg(u) = the number of stored outgoing entries of u.  Rank flows along outgoing entries and is PULLED
 *             over the incoming CSR; symmetric = 1: the caller vouches that the stored graph is symmetric, and the outgoing CSR serves as both (the
 *             rule of vgl_hip_lp_run, vgl_hip_bc_run and vgl_hip_msbfs_run).
 *   problems  `count` seed lists on the host: list j is seeds[seed_ptr[j] .. seed_ptr[j + 1]) in the graph's numbering.  p_j = seed_weight over the
 *             list divided by its sum, the sum added in list order in float64 (seed_weight NULL: 1 each); a vertex listed twice gets both weights.
 *             An EMPTY list means p_j = 1 / V on every vertex: plain PageRank.
 *   iteration from x_0 = p:   y[u] = x[u] / (double)outdeg(u), 0 for a dangling u (outdeg 0);   D = the sum of x[u] over the dangling u;
 *                             x'[v] = alpha * (the sum of y[u] over the incoming entries (u -> v)) + (alpha * D + 1 - alpha) * p[v];
 *             err = the sum over v of |x'[v] - x[v]|.  This is networkx's pagerank with dangling = personalization.
 *   stopping  problems run in batches of up to 16, in the given order: batch k is list 16 k .. 16 k + 15, the last may be partial.  tol == 0: a batch
 *             runs exactly max_iterations iterations and nothing is read back between them.  tol > 0: a batch stops after the first iteration
 *             whose largest err over its columns is <= tol, or at max_iterations: one read of the pinned counter mirror per iteration.  Columns
 *             that converge early keep iterating with their batch.  max_iterations == 0 returns p.
 *   outputs   d_rank: count x V float64, source-major, indexed with int64 (like d_levels of vgl_hip_msbfs_run); d_err (optional, count float64): each
 *             problem's last err (0 without an iteration); d_iterations (optional, count int32): the iterations its batch ran.
 *   floating point: float64 throughout, -ffp-contract=off, no fast-math, NO floating-point atomic anywhere.  Every value has one writer, and every
 *             sum (a row's pull, D, err) has a fixed shape that is a function of the graph, the position of the column in its batch, the batch's
 *             width and the run-time switches only: the same call returns the same bits on every run.  Across switches, batch widths and
 *             positions in a batch the results agree within the tolerance below, NOT bit for bit.
 *   tolerance all terms are non-negative, so one evaluation of the map has a relative error of at most gamma_k = k u / (1 - k u) per component,
 *             u = 2^-53, k = max(largest in-degree, number of dangling vertices) + 6 (the roundings on the longest chain into one value: the sum, and
 *             the division, the scaling by alpha, alpha * D, + (1 - alpha), * p[v] and the teleport addition); the map contracts by alpha in L1 on
 *             vectors of mass 1, so after t iterations  |computed - exact|_1 <= gamma_k (1 - alpha^t) / (1 - alpha).  Two float64 evaluations differ by
 *             at most twice that.
 * Method: per batch the state is VERTEX-MAJOR, V x W float64 with W in {1, 4, 16} the smallest width that holds the batch (unused columns are 0), so a
 * vertex's W values are contiguous (W = 16: one 128-byte line) and a lane loads 16 bytes (two columns) where W >= 2.  One pull kernel per row class
 * of the pull direction (VGL_PPR_SHORT 32: 8 lanes per row, VGL_PPR_WAVE 1024: a wavefront, longer: one workgroup per VGL_PPR_CHUNK 16384 entries; the
 * lanes are entry slot x column pair, the slots folded by shuffles and, across a workgroup, in LDS in wave order; the chunk sums of a row of more than
 * one chunk are added in chunk order by one writer).  The writer of (v, column) scales by alpha, stores x', stores y' = x' / outdeg by one IEEE
 * division and takes the terms of err and D.  A listed p is added at the batch's seed vertices alone; the uniform p is added in the epilogue.  Every
 * workgroup leaves its err and D terms at a place of its own, and one workgroup folds them in a fixed order, leaves alpha D + 1 - alpha for the next
 * iteration and publishes the largest err.  A last kernel transposes the batch into d_rank.  The class lists (in ascending order inside a class) and
 * the chunk table are built per direction by vgl_hip_ppr_prepare or the first run, cached on the handle and freed with it.
 * stats: sources = problems run; batches = ceil(count / 16); iterations_total = the sum over the batches of the iterations run, iterations_max the
 * largest; batches_converged = batches that the tolerance stopped (tol > 0 and the largest err <= tol, at max_iterations too); prepared_now = this call
 * built lists; entries_walked = the sum over the batches of iterations x incoming entries: exact; max_err = the largest last err of a problem;
 * algorithmic_bytes = per batch (16 W + 9) V (x and y = p written, the outgoing row bounds and the seed mark read) + per iteration
 * E (4 + 8 W) (the adjacency entry and the W values of its far end) + V (21 + 24 W) (the list entry 4, the row bounds of both directions 8 + 8, the
 * seed mark 1, x read, x' and y' written) + 8 V (W + nb) (the transpose: the batch read, nb rows written); the seeds, the partial sums and what the
 * caches serve are left out: a lower bound.
 * Fails, before any output is written: a sharded handle, no incoming CSR without symmetric = 1, alpha not finite or outside [0, 1), tol not finite or
 * < 0, max_iterations < 0, count < 0, a seed_ptr that decreases, a seed outside [0, V), a seed weight that is not finite or <= 0, d_rank NULL.
 * count == 0 succeeds and writes nothing.
 * Not here: edge weights (the handle keeps no map from an outgoing entry to its incoming position), reverse PageRank, top-k extraction, forward push
 * and other local methods, freezing converged columns, more than one GPU. */
typedef struct {
    int32_t sources;            /* problems run */
    int32_t batches;            /* groups of up to 16 problems */
    int32_t iterations_max;     /* most iterations of a batch */
    int32_t batches_converged;  /* batches that the tolerance stopped */
    int32_t prepared_now;       /* this call built the class lists */
    int64_t iterations_total;   /* sum over the batches of the iterations run */
    int64_t entries_walked;     /* sum over the batches of iterations x incoming entries: exact */
    int64_t algorithmic_bytes;
    double max_err;             /* largest last err of a problem */
} vgl_hip_ppr_stats;
int vgl_hip_ppr_prepare(vgl_hip_ctx *ctx, vgl_hip_graph *g, int symmetric);
int vgl_hip_ppr_run(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *seeds, const int64_t *seed_ptr, const double *seed_weight, int32_t count,
                    double alpha, int32_t max_iterations, double tol, int symmetric, double *d_rank, double *d_err, int32_t *d_iterations,
                    vgl_hip_ppr_stats *stats);

/* Neighbour aggregation with gradients (`agg`): for every row of a CSR, the sum, mean, max or min of the feature rows of its entries, float32, any
 * width, optionally weighted per entry, and the exact backward of that step.  It is what consumes the blocks of vgl_hip_sample_neighbors, and the
 * general form of the fixed-width pull of vgl_hip_ppr_run.  The reference has no counterpart, so this comment is the contract:
 *   plan      vgl_hip_agg_plan_create BORROWS a device CSR: d_rowptr int64 [n_rows + 1] with rowptr[0] = 0 that does not decrease, d_adj int32
 *             [rowptr[n_rows]] with every entry in [0, n_cols).  The CSR need not belong to a handle: the stored arrays of either direction of a
 *             graph serve as they are (n_rows = n_cols = V), and so do the rowptr / adj of a sampled block.  Entries are taken AS STORED: a repeated
 *             entry counts as often as it is stored, a self entry is an entry like any other.  The arrays must outlive the plan and must not change.
 *             The plan checks its input (a count over the rows, a count over the entries), classifies the rows once (VGL_AGG_SHORT 32: 8 lanes per
 *             row, empty rows among them; VGL_AGG_WAVE 1024: a wavefront; longer: a workgroup per chunk of VGL_AGG_CHUNK 16384 entries, the chunk
 *             raised until the longest row has at most 32768), and keeps each class list in ascending order.  At most 2^31 - 16 entries.
 *             vgl_hip_agg_plan_info returns the stats of the plan (the run fields 0); _destroy frees what the plan owns, nothing that it borrowed.
 *   transpose built by the first vgl_hip_agg_run_transposed of a plan and kept in it: the CSR with n_cols rows whose row u lists, IN ASCENDING ENTRY
 *             POSITION p, the entries with adj[p] = u; for each it holds row(p) and the origin p.  It comes from the stable vgl_hip_coo_to_csr (with
 *             d_perm) over the entry list in CSR order, and has class lists and chunks of its own.
 *   forward   vgl_hip_agg_run: x is n_cols x F float32, row-major with leading dimension ldx >= F (in elements), out n_rows x F with ldo >= F,
 *             d_weight one float32 per entry in CSR order or NULL (1 each), F >= 1 without an upper limit besides memory.
 *               VGL_HIP_AGG_SUM   out[i, f] = the sum over the entries p of row i of w_p * x[adj[p], f]
 *               VGL_HIP_AGG_MEAN  that sum divided once by (float) len(i); an empty row gives 0
 *               VGL_HIP_AGG_MAX / _MIN  the extreme of x[adj[p], f] over the row; d_arg[i, f] (int32, n_rows x F, leading dimension F, optional) = the
 *                                 SMALLEST position p that attains it; an empty row gives 0 and -1.  No weights.  With a NaN in x the result of MAX /
 *                                 MIN (value and arg) is UNSPECIFIED.
 *   backward  vgl_hip_agg_run_transposed: g is n_rows x F (ldg), gx n_cols x F (ldgx);  gx[u, f] = the sum over the transposed row of u, in its order,
 *             of coefficient(p) * g[row(p), f], with coefficient w_p (1 without weights) for SUM, w_p / (float) len(row(p)) for MEAN (one division,
 *             then one product), and for MAX / MIN 1 if d_arg[row(p), f] == p else 0 (d_arg: what the forward run wrote).  The weight and the arg are
 *             read through the origin p: no permuted copy of the weights is made.  This is the gradient of the forward with respect to x.
 *   floating point: float32 accumulation, -ffp-contract=off, no fast-math, IEEE division, NO floating-point atomic; every output value has one
 *             writer.  Every sum has a shape that is a function of (row length, F, VEC, the three switches) only, where VEC is 4 when F, every
 *             leading dimension and every base address of the call are multiples of 4 elements / 16 bytes and 1 otherwise: the same call returns
 *             the same bits on every run.  Across switch settings and VEC results agree within the tolerance, NOT bit for bit; on data whose partial
 *             sums are all exact in float32 (small integers) every shape gives the same bits.  The arg does not depend on the shape at all.
 *   tolerance per output value, with d terms c_p * v_p:  |computed - exact| <= gamma_k * the sum of |c_p * v_p|, k = d + 2, gamma_k = k u / (1 - k u),
 *             u = 2^-24: one rounding per product, at most d - 1 additions on a chain whatever the shape, one division for MEAN and one more
 *             product for its backward.
 * Method: one team kernel for both passes; a team's lanes are (entry slot x column group): NQ lanes (a power of two, at most 8 in the short class and
 * 64 in the others) cover a tile of NQ * VEC columns, slot s adds entries s, s + SLOTS, ... in row order with four gathers in flight, the slots of a
 * column group are folded by an xor butterfly and a workgroup's four waves from LDS in wave order.  A wider F walks the row once per column tile and
 * reads adj again.  A row of more than one chunk leaves a partial per chunk (for MAX / MIN a value and a position per column), and one writer per
 * (row, column) finishes them in chunk order, the smaller position winning a tie.
 * stats: rows, entries = of the CSR walked (the plan's, or the transpose: n_cols rows); rows_short / _wave / _wg its rows per class; chunks = the
 * workgroup class's items; hub_rows = rows of more than one chunk; column_tiles[class] = walks per row; vec; transposed = 1 for the backward run (in
 * _plan_info: the transpose exists).  algorithmic_bytes = per class entries x column_tiles x (4 adjacency + 4 with weights [+ 4 origin, + 16 the
 * bounds of row(p) for MEAN, in the transposed run]): what is REQUESTED, the walks after the first are served by the caches, so this term is an upper
 * bound of what memory sees; + entries x 4 F gathered (twice with the arg of a transposed MAX / MIN): requested bytes, a lower bound where rows are
 * not aligned to lines and an upper bound of the memory traffic where a feature row is re-read from cache; + rows x (8 bounds + 4 F written + 4 F with
 * d_arg): exact; + the list entry, 4 per short or wave row and 8 per chunk: exact.  The chunk partials are left out.
 * Fails, before anything is written: a NULL argument, a negative size, a rowptr that does not start at 0 or decreases, an entry outside [0, n_cols),
 * more than 2^31 - 16 entries; F < 1, a leading dimension below F, an op outside the four, a weight with MAX / MIN, a transposed MAX / MIN run without
 * d_arg, a plan of another context.
 * Threads: every entry point makes the context's device current itself (a backward pass arrives on a thread of its own).  The pinned counter mirror
 * is per context: one call at a time per context.
 * Not here: float16 / bfloat16 features, a fused dense transform, more than one GPU.  Gradients with respect to the entry weights are
 * vgl_hip_agg_sddmm below (the section on edge scores). */
enum { VGL_HIP_AGG_SUM = 0, VGL_HIP_AGG_MEAN = 1, VGL_HIP_AGG_MAX = 2, VGL_HIP_AGG_MIN = 3 };
typedef struct vgl_hip_agg_plan vgl_hip_agg_plan;
typedef struct {
    int64_t rows;               /* rows of the CSR walked */
    int64_t entries;
    int64_t rows_short, rows_wave, rows_wg;
    int64_t chunks;             /* items of the workgroup class */
    int64_t hub_rows;           /* rows of more than one chunk */
    int64_t algorithmic_bytes;
    int32_t column_tiles[3];    /* walks per row of the short, wave and workgroup class */
    int32_t vec;                /* 4: 16-byte loads and stores; 1: scalar */
    int32_t transposed;         /* the run walked the transpose (plan_info: it exists) */
    int32_t heads;              /* H of the _heads calls (below); 0 from every other call */
} vgl_hip_agg_stats;
int vgl_hip_agg_plan_create(vgl_hip_ctx *ctx, const int64_t *d_rowptr, const int32_t *d_adj, int32_t n_rows, int32_t n_cols, vgl_hip_agg_plan **out);
int vgl_hip_agg_plan_info(vgl_hip_agg_plan *plan, vgl_hip_agg_stats *stats);
int vgl_hip_agg_plan_destroy(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan);
int vgl_hip_agg_run(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, int op, const float *d_weight, const float *d_x, int64_t ldx, int32_t F, float *d_out,
                    int64_t ldo, int32_t *d_arg, vgl_hip_agg_stats *stats);
int vgl_hip_agg_run_transposed(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, int op, const float *d_weight, const int32_t *d_arg, const float *d_g,
                               int64_t ldg, int32_t F, float *d_gx, int64_t ldgx, vgl_hip_agg_stats *stats);

/* Edge scores, edge softmax (`edge`): one float32 per stored entry of a vgl_hip_agg_plan, in CSR order.  With vgl_hip_agg_run / _run_transposed they
 * close the gradients of a weighted aggregation and make graph attention three calls.  The reference has no counterpart, so this comment is the
 * contract:
 *   sddmm     vgl_hip_agg_sddmm: a is n_rows x F float32 (leading dimension lda >= F, in elements), b n_cols x F (ldb >= F), e one float32 per entry;
 *             e[p] = the sum over f of a[row(p), f] * b[adj[p], f]; with mean = 1 that sum divided once by (float) len(row(p)).  It is the score of
 *             dot-product attention, and the gradient of vgl_hip_agg_run with respect to d_weight: a = the gradient of out, b = x, mean = 1 for
 *             VGL_HIP_AGG_MEAN.  Its own gradients need no further kernel: with ge per entry, ga = vgl_hip_agg_run(SUM, weight = ge, x = b) and
 *             gb = vgl_hip_agg_run_transposed(SUM, weight = ge, g = a).
 *   softmax   vgl_hip_agg_edge_softmax: per row i, over the entries p of the row, m = the largest e[p], s = the sum of expf(e[p] - m),
 *             y[p] = expf(e[p] - m) / s: ONE DIVISION per entry, no reciprocal, so a row of d equal scores gives exactly 1 / (float) d.  An entry at
 *             -inf gets y = 0 exactly; a row whose entries are all -inf gets y = 0 everywhere; an empty row writes nothing.  With a NaN or +inf in e the
 *             result is UNSPECIFIED.  d_y must not overlap d_e.
 *   backward  vgl_hip_agg_edge_softmax_backward: ge[p] = y[p] * (gy[p] - d), d = the sum over the row's entries q of y[q] * gy[q].  It is this formula
 *             on ANY y, a softmax output or not.  d_ge must not overlap d_y or d_gy.
 *   floating point: as above (float32, -ffp-contract=off, expf of the device library, IEEE division, NO floating-point atomic, one writer per value).
 *             A dot product has the shape: a lane adds its VEC products in column order, tile after tile; the NQ lanes of an entry are folded by an
 *             xor butterfly at offsets 1, 2, ... NQ / 2.  It depends on (F, VEC, the entry's class) only: chunks and slots only divide the work.  A
 *             row sum of the softmax and of its backward has the shape: lane s of the team (8 / 64 / 256 lanes) adds entries s, s + LANES, ... of the
 *             row or chunk in order; an xor butterfly at offsets 1, 2, ... folds the lanes of a wave; a workgroup adds its four waves in wave order; a
 *             row of more than one chunk leaves (m_c, s_c) per chunk and ONE thread merges them in chunk order, M = max m_c,
 *             S = the sum of s_c * expf(m_c - M) (a chunk whose entries are all -inf has s_c = 0 and contributes 0; no -inf - -inf is formed); the
 *             backward's d is the sum of the d_c in chunk order.  The same call returns the same bits on every run.
 *   tolerance  dot: gamma_(F + 2) * the sum of |a b|.  backward: gamma_(d + 3) * |y_p| * (|gy_p| + the sum of |y_q gy_q|), d the row
 *             length.  forward, relative to the exact y_p: 3 (R u + eps_exp) + gamma_(d + 3), plus 2^-126 absolute, R = the largest |e - m| of the row,
 *             eps_exp the measured error of expf (tests/studies/expf_ulps.hip).
 * Method: vgl_k_edge_dot<CLS, VEC> runs over the plan's forward class lists with the lane layout of the aggregation (entry slot x column group, four
 * gathers of b in flight); the row's a stays in registers with one column tile and is re-read per tile from cache with more.  No fold over slots, no
 * chunk partials.  vgl_k_edge_rows<CLS, BWD>: every lane an entry slot; rows of one chunk finish in one launch (walks: max, sum, write; backward: sum,
 * write); rows of more chunks take three: partials, vgl_k_edge_hubs (one thread per hub row), vgl_k_edge_hub_write over the workgroup items.
 * VEC = 4 when F, lda, ldb are multiples of 4 and d_a, d_b are 16-byte aligned, else 1.
 * stats: rows, entries, rows_short / _wave / _wg, chunks, hub_rows = of the plan's CSR; column_tiles, vec as in vgl_hip_agg_run (softmax: 1, 1);
 * transposed = 0.  algorithmic_bytes:
 *   sddmm    per class entries x column_tiles x 4 (adjacency; requested: the tiles after the first come from cache, an upper bound)
 *            + entries x 4 F (b gathered; requested, as for vgl_hip_agg_run) + entries x 4 (e written; exact)
 *            + rows x (8 bounds + 4 F of a) (a lower bound with more than one tile or slot group: a is re-read from cache) + the list entries (4 per
 *            short or wave row, 8 per chunk; exact).
 *   softmax  entries x (4 x 3 walks of e + 4 written): the walks after the first are requested, not memory traffic (a chunk is 64 KiB): upper bound
 *            + rows x 8 + the list entries (exact).  The hub partials are left out.
 *   backward entries x (8 x 2 walks of y and gy + 4 written) + rows x 8 + the list entries; the same remarks.
 * Fails, before anything is written: a NULL argument (stats may be NULL), a plan of another context, F < 1, a leading dimension below F, mean outside
 * {0, 1}.  Threads: as above.
 * Not here: a fused attention that never materialises the E scalars (they are 12 bytes per entry against 8 F); a softmax grouped by column;
 * float16 / bfloat16.  Heads are the _heads calls below; the u_add_v score of the original GAT is vgl_hip_agg_edge_add_heads further down. */
int vgl_hip_agg_sddmm(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_a, int64_t lda, const float *d_b, int64_t ldb, int32_t F, int mean,
                      float *d_e, vgl_hip_agg_stats *stats);
int vgl_hip_agg_edge_softmax(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_e, float *d_y, vgl_hip_agg_stats *stats);
int vgl_hip_agg_edge_softmax_backward(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_y, const float *d_gy, float *d_ge,
                                      vgl_hip_agg_stats *stats);

/* Heads (`heads`): the five calls above with H heads in one walk.  F is the total width, F % H == 0, D = F / H; head h owns the
 * columns [h D, (h + 1) D) of every feature matrix.  The edge scalars are ONE float32 per (entry, head), E x H row-major and contiguous:
 * e[p * H + h], p the entry's position in CSR order; they have no leading dimension.  For every head h, entry p and column f with f / D == h:
 *   sddmm     vgl_hip_agg_sddmm_heads: e[p, h] = the sum over the columns f of head h of a[row(p), f] * b[adj[p], f]; with mean = 1 divided once by
 *             (float) len(row(p)).
 *   softmax   vgl_hip_agg_edge_softmax_heads / _backward_heads: the formulas, the -inf rules, the empty rows, the one division per entry and the
 *             overlap conditions of the calls above, per (row, head) on column h of e.
 *   forward   vgl_hip_agg_run_heads: out[i, f] = the sum over the entries p of row i of w[p, h] * x[adj[p], f]; MEAN divides once by the row's length.
 *   backward  vgl_hip_agg_run_transposed_heads: gx[u, f] = the sum over the transposed row of u, in its order, of coef * g[row(p), f], coef = w[p, h]
 *             for SUM and w[p, h] / (float) len(row(p)) for MEAN (one division, then one product); the weight is read through the origin.
 *   floating point: everything above stands.  VEC = 4 when D, every leading dimension and every base address are multiples of 4 elements / 16 bytes
 *             (a 16-byte access then stays inside one head), else 1.  The dot product of (entry, head) has the shape vgl_hip_agg_sddmm gives at width
 *             D on the column slice of the head: lanes per tile and tiles from (D, VEC), the butterfly over the lanes of that head only, so e[:, h]
 *             equals vgl_hip_agg_sddmm on a[:, h D : (h + 1) D], b[:, h D : (h + 1) D] BIT FOR BIT.  Every row sum of the softmax and of its backward
 *             has the shape above per head, one thread per (hub row, head) merges the chunks in chunk order: y[:, h] equals the call above on a
 *             contiguous copy of e[:, h] BIT FOR BIT.  The two runs keep the sum of the width-F call (slots and tiles from (F, VEC)); only the
 *             coefficient depends on the lane's head: with H equal weight columns and the same VEC they return the bits of vgl_hip_agg_run /
 *             _run_transposed with that column as the weight.  With H = 1 every call returns the bits of its counterpart above.
 *   tolerance the ones above with D in place of F for the dot: gamma_(D + 2) * the sum of |a b|; the softmax bounds unchanged; the runs
 *             gamma_(d + 2) * the sum of |w v|.
 * Method: vgl_k_edge_dot_heads<CLS, VEC>: the lanes of an entry slot are (head of the pass x column group of the head); NQ_D lanes per head from
 * (D, VEC), as many heads beside each other as the class's lane budget holds (8 short, 64 otherwise; a power of two, no more than H needs), the
 * remaining heads in further passes; adj[p] is read once per entry for all passes; the butterfly stops at NQ_D / 2 and the lane of column group 0
 * stores e[p * H + h].  vgl_k_edge_rows_heads<CLS, BWD, HB>: every lane an entry slot that carries a block of HB heads (the largest of 8, 4, 2, 1
 * that divides H) in registers and loads them as one 8- or 16-byte access when the arrays are 16-byte aligned, a loop over the blocks; the hub
 * partial is a pair per (item, head), one thread per (hub row, head) merges.  vgl_k_agg_rows<..., HEADS>: the walk of vgl_hip_agg_run, the
 * coefficient weight[o * H + c0 / D] with the head taken once per column tile.
 * stats: as above, heads = H.  column_tiles: sddmm: passes x the tiles of a head per class; softmax: 1; the runs: those of (F, VEC).  vec: the VEC
 * above; softmax: 4 where a lane's head block is read in 16-byte pieces, else 1.  algorithmic_bytes:
 *   sddmm    per class entries x column_tiles x 4 (adjacency; REQUESTED as above: the kernel keeps adj[p] in a register, an upper bound)
 *            + entries x 4 F (b gathered) + entries x 4 H (e written) + rows x (8 bounds + 4 F of a) + the list entries (4 per short or wave
 *            row, 8 per chunk).
 *   softmax  entries x H x (4 x 3 + 4) + rows x 8 + the list entries.   backward  entries x H x (8 x 2 + 4) + rows x 8 + the list entries.
 *   runs     the formula of vgl_hip_agg_run / _run_transposed with 4 H of weights per entry and per walk in place of 4.
 * Fails, before anything is written: what the calls above refuse; H < 1; F % H != 0; a NULL d_weight; an op other than SUM or MEAN in the runs.
 * Not here: a leading dimension for the E x H arrays; the fused attention; float16 / bfloat16. */
int vgl_hip_agg_sddmm_heads(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_a, int64_t lda, const float *d_b, int64_t ldb, int32_t F, int32_t H,
                            int mean, float *d_e, vgl_hip_agg_stats *stats);
int vgl_hip_agg_edge_softmax_heads(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_e, int32_t H, float *d_y, vgl_hip_agg_stats *stats);
int vgl_hip_agg_edge_softmax_backward_heads(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_y, const float *d_gy, int32_t H, float *d_ge,
                                            vgl_hip_agg_stats *stats);
int vgl_hip_agg_run_heads(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, int op, const float *d_weight, int32_t H, const float *d_x, int64_t ldx, int32_t F,
                          float *d_out, int64_t ldo, vgl_hip_agg_stats *stats);
int vgl_hip_agg_run_transposed_heads(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, int op, const float *d_weight, int32_t H, const float *d_g, int64_t ldg,
                                     int32_t F, float *d_gx, int64_t ldgx, vgl_hip_agg_stats *stats);

/* The additive score of GAT and the entry sums (`gat`): the u_add_v score act(s[row(p)] + t[adj[p]]) of the original graph
 * attention layer on the E x H layout above, and the two reductions that are its gradients.  A single head is H = 1.  With the softmax and the run of
 * the heads section they make the GAT layer three calls.  The reference has no counterpart, so this comment is the contract:
 *   score     vgl_hip_agg_edge_add_heads: s is n_rows x H float32 (leading dimension lds >= H, in elements), t n_cols x H (ldt >= H), e E x H
 *             contiguous in CSR order.  z = s[row(p), h] + t[adj[p], h]: ONE float32 addition;  e[p, h] = z > 0 ? z : slope * z: ONE float32 product
 *             (LeakyReLU; slope is a float, slope = 1 is the identity on bits, slope = 0 is ReLU).  Exactly one of d_s, d_t may be NULL: the term is
 *             then ABSENT and nothing is added, z = t[adj[p], h] or z = s[row(p), h] with its bits (a -0 stays -0): the two broadcasts "copy a row
 *             value / a column value onto its entries".  With a NaN or an infinity in s or t the result is UNSPECIFIED.
 *   sums      vgl_hip_agg_edge_sum_heads: w is E x H, gate E x H or NULL.  c(p, h) = w[p, h] when gate is NULL or gate[p, h] > 0, otherwise
 *             slope * w[p, h]: ONE product.  This is the derivative of the activation above as torch defines it (slope at 0), applied on the fly;
 *             because slope >= 0 the score itself serves as the gate.  transposed = 0: out[i, h] = the sum of c(p, h) over the entries p of row i,
 *             out n_rows x H with ldo >= H.  transposed = 1: out[u, h] = the sum over the transposed row of u, in its order, of c(origin, h): w and
 *             gate are read through the origin as vgl_hip_agg_run_transposed reads its weight, out is n_cols x H; the transpose is built on first
 *             use and kept.  An empty row gives 0.  With ge the gradient of e: gs = the sum (gate = e) and gt = the transposed sum (gate = e); the
 *             gradient of a sum is the score with one term absent and slope 1, so the pair closes under differentiation.
 *   floating point: as above (float32, -ffp-contract=off, NO floating-point atomic, one writer per value).  The score has at most two roundings per
 *             value and no sum: it has no shape, and equals the float32 restatement BIT FOR BIT on every class, switch setting and alignment.  A sum
 *             has the shape of the softmax's row sums: lane s of the team (8 / 64 / 256 lanes) adds entries s, s + LANES, ... of the row or chunk in
 *             order; an xor butterfly at offsets 1, 2, ... folds the lanes of a wave; a workgroup adds its four waves in wave order; a row of more
 *             than one chunk leaves one float per (item, head) and ONE thread per (hub row, head) adds them in chunk order and writes the result.
 *             The shape is a function of (row length, the three switches) only: the same call returns the same bits on every run, and on data whose
 *             partial sums are all exact every setting returns the same bits.
 *   tolerance per value of a sum with d terms:  |computed - exact| <= gamma_k * the sum of |c(p, h)|, k = d, gamma_k = k u / (1 - k u), u = 2^-24: one
 *             rounding for the product of a gated term, at most d - 1 additions on a chain whatever the shape (an addition of a lane without
 *             entries adds an exact 0); c in the bound is the exact product.
 * Method: vgl_k_edge_add_heads<CLS, HB> over the plan's forward class lists: every lane an entry slot that carries a block of HB heads (the largest of
 * 8, 4, 2, 1 that divides H), four entries in flight; adj[p] is read once per entry and kept across the blocks; the row's s block stays in registers
 * where one block covers H and is re-read per block from cache otherwise; a block of s, t, e moves as one 8- or 16-byte access where the base
 * address is 16-byte aligned and the leading dimension a multiple of 4 elements (2 for a block of two), else scalar.  No fold, no LDS, no hub stage.
 * vgl_k_edge_sum_heads<CLS, GATE, TR, HB>: the walk and fold of the softmax backward's row sum, with TR over the transpose through t_origin; the
 * lead lane writes a row of one chunk; vgl_k_edge_sum_hubs finishes the rows of more chunks.
 * stats: heads = H; column_tiles = 1 / 1 / 1; vec = 4 where a lane's head block moves in 16-byte pieces in every array of the call (HB >= 4), else
 * 1; transposed as passed; rows, entries, rows_short / _wave / _wg, chunks, hub_rows = of the CSR walked (the transpose: n_cols rows).
 * algorithmic_bytes:
 *   score    entries x (4 adjacency + 4 H of t gathered when d_t is given + 4 H of e written) + rows x (8 bounds + 4 H of s when d_s is given) + the
 *            list entries (4 per short or wave row, 8 per chunk).  The gather is requested bytes, as for vgl_hip_agg_run; without d_t the kernel
 *            does not read the adjacency and that term is an upper bound.
 *   sums     entries x (4 H of w + 4 H of the gate when given + 4 of the origin when transposed) + rows x (8 bounds + 4 H written) + the list
 *            entries.  The chunk partials are left out.
 * Fails, before anything is written: a NULL ctx, plan, d_e / d_out or d_w; d_s and d_t both NULL; a plan of another context; H < 1; a leading
 * dimension below H; a slope that is negative, NaN or infinite; transposed outside {0, 1}; an output that overlaps an input.  stats may be NULL.
 * Threads: as above.
 * Not here: a fused score + softmax + sum that never materialises E x H; GATv2 (the activation before a second dot product); a softmax grouped by
 * column; float16 / bfloat16; a leading dimension for the E x H arrays. */
int vgl_hip_agg_edge_add_heads(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_s, int64_t lds, const float *d_t, int64_t ldt, int32_t H,
                               float slope, float *d_e, vgl_hip_agg_stats *stats);
int vgl_hip_agg_edge_sum_heads(vgl_hip_ctx *ctx, vgl_hip_agg_plan *plan, const float *d_w, const float *d_gate, float slope, int32_t H,
                               int transposed, float *d_out, int64_t ldo, vgl_hip_agg_stats *stats);

/* ---- super-step pieces for the edge-cut multi-GPU path (one process per GPU; the exchange between steps is an
 *      RCCL collective issued by the host side, replacing common/mpi_exchange.hpp:110-150,222-271) ---- */
int vgl_hip_bfs_init(vgl_hip_ctx *ctx, int32_t V, int32_t source, int32_t *d_levels);
/* expand the owned part of level `level`: frontier = owned rows with levels == level.  Writes levels[dst] = level+1
 * anywhere in the replicated array.  d_visited_bits: replicated visited bitmap (V bits) or NULL to have it rebuilt from
 * levels.  local_frontier/local_edges are host outputs (the frontier is compacted before the expand, which is left enqueued). */
int vgl_hip_bfs_step_top_down(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_levels, int32_t level,
                              const uint64_t *d_visited_bits, int64_t *local_frontier, int64_t *local_edges);
/* bottom-up step over the owned rows (needs the incoming CSR): unvisited owned vertices with an in-neighbour in the frontier
 * bitmap get levels = level+1.  d_next_bits (V bits) receives exactly this rank's discoveries (other words zero), ready for
 * the bitmap exchange.  found / probed (optional, synchronise): discovered vertices, adjacency entries examined. */
/* top-down step driven by the replicated bitmaps: the owned part of the frontier is read from d_front_bits (V/64 words instead
 * of a scan of levels), every vertex this shard discovers gets levels[v] = level+1 and its bit in d_next_bits (cleared here,
 * full length: destinations live in any shard).  d_next_bits is what the shard contributes to the exchange. */
int vgl_hip_bfs_step_top_down_bits(vgl_hip_ctx *ctx, vgl_hip_graph *graph, int32_t *d_levels, int32_t level,
                                   const uint64_t *d_visited_bits, const uint64_t *d_front_bits, uint64_t *d_next_bits,
                                   int64_t *local_frontier, int64_t *local_edges);
/* out[w] = OR over p < parts of in[p * words + w]  (merging the bitmap slices a rank received in the two-phase exchange) */
int vgl_hip_bitmap_or_parts(vgl_hip_ctx *ctx, int64_t words, int parts, const uint64_t *d_in, uint64_t *d_out);
int vgl_hip_bfs_step_bottom_up(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_levels, int32_t level,
                               const uint64_t *d_visited_bits, const uint64_t *d_front_bits, uint64_t *d_next_bits,
                               int64_t *found, int64_t *probed);
/* The frontier bitmap folded onto 2^17 bits, as the fused traversal's filtered bottom-up probe reads it (VGL_BFS_FILTER_F):
 * d_fold[j] = OR over k of d_front[j + 2048 * k] for j in 0 .. 2047; words of d_front at and past `words` count as 0.  All 2048 words of
 * d_fold are written.  Asynchronous on the context's stream. */
int vgl_hip_bfs_front_fold(vgl_hip_ctx *ctx, int64_t words, const uint64_t *d_front, uint64_t *d_fold);
/* bitmap (V bits, little-endian within uint64 words) of vertices with d_levels == level */
int vgl_hip_levels_to_bitmap(vgl_hip_ctx *ctx, int32_t V, const int32_t *d_levels, int32_t level, uint64_t *d_bits);
/* OR `parts` bitmaps (each V/64 words, contiguous) and set levels[v] = level where a bit is set and v is unvisited.
 * Optional replicated state for the next direction decision: d_visited_bits |= new frontier, d_front_bits = new frontier,
 * d_degrees (int32[V] out-degrees of ALL vertices) -> *newly_degree = sum of the new frontier's out-degrees.
 * *newly = number of vertices that now have d_levels == level.  Synchronises. */
int vgl_hip_bfs_apply_bitmaps(vgl_hip_ctx *ctx, int32_t V, int parts, const uint64_t *d_bits_all, int32_t *d_levels, int32_t level,
                              uint64_t *d_visited_bits, uint64_t *d_front_bits, const int32_t *d_degrees, int64_t *newly,
                              int64_t *newly_degree);
/* vgl_hip_bfs_apply_bitmaps for a rank that keeps levels only for the rows it owns: the replicated bitmaps are updated for every vertex
 * (any rank may probe any vertex), d_levels / the two results only for [own_begin, own_end) (multiples of 64) -- the per-vertex part
 * of the merge no longer grows with the whole graph on every rank; the caller adds the two results over the ranks. */
int vgl_hip_bfs_apply_bitmaps_owned(vgl_hip_ctx *ctx, int32_t V, int parts, const uint64_t *d_bits_all, int32_t *d_levels, int32_t level,
                                    uint64_t *d_visited_bits, uint64_t *d_front_bits, const int32_t *d_degrees, int32_t own_begin,
                                    int32_t own_end, int64_t *newly_owned, int64_t *newly_owned_degree);
/* Sparse exchange of tiny levels (the id-list counterpart of the bitmap exchange of common/mpi_exchange.hpp:222-271):
 * d_out[0] = number of set bits of the bitmap (may exceed cap), d_out[1 .. 1+cap) = ids of (the first cap of) them, unordered.
 * Asynchronous on the context's stream. */
int vgl_hip_bitmap_to_ids(vgl_hip_ctx *ctx, int64_t words, const uint64_t *d_bits, int32_t cap, int32_t *d_out);
/* vgl_hip_bfs_apply_bitmaps for `parts` id lists of that layout (stride 1 + cap, every count <= cap): unvisited listed vertices get
 * d_levels = level, their visited bits are set and d_front_bits becomes exactly the set of them.  Synchronises. */
int vgl_hip_bfs_apply_ids(vgl_hip_ctx *ctx, int32_t V, int parts, int32_t cap, const int32_t *d_lists, int32_t *d_levels, int32_t level,
                          uint64_t *d_visited_bits, uint64_t *d_front_bits, const int32_t *d_degrees, int64_t *newly,
                          int64_t *newly_degree);
int vgl_hip_sssp_init(vgl_hip_ctx *ctx, int32_t V, int32_t source, float *d_dist);
/* one all-active push relaxation over the owned rows; *changed = 1 if any distance decreased. Synchronises. */
int vgl_hip_sssp_relax_owned(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_weights, float *d_dist, int *changed);
int vgl_hip_cc_init(vgl_hip_ctx *ctx, int32_t V, int32_t *d_comp);
int vgl_hip_cc_hook_owned(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_comp, int *changed);
int vgl_hip_cc_jump(vgl_hip_ctx *ctx, int32_t V, int32_t *d_comp);
/* PageRank pieces: prepare (contrib = old*rdeg, dangling sum over ALL vertices) and pull over the owned rows only;
 * ranks of owned rows are written, the caller all-gathers owned slices (EXCHANGE_PRIVATE_DATA, pr.hpp:127). */
int vgl_hip_pr_setup(vgl_hip_ctx *ctx, int32_t V, const int32_t *d_indeg_noloops, float *d_ranks, float *d_rdeg);
/* The sum-type all-active advance of PR::vgl_page_rank (algorithms/pr/pr.hpp:105-124: `page_ranks[src] += contribution[dst]` over every edge
 * src -> dst with dst != src) with the caller's own arrays: d_sums[src] = sum over those edges of d_values[dst], for the rows the handle owns.
 * Runs as the blocked pass (values read from LDS windows, exact 64-bit fixed-point accumulation, rounded to f32 once: the same bits for any
 * schedule; it differs from an f32 `+=` chain in adjacency order by the chain's own rounding).  The layout is the one
 * vgl_hip_pr_prepare(BLOCKED) builds (built here on first use).  Asynchronous on the context's stream.
 * The fixed point: with sum_bound = m * 2^e, 0.5 <= m < 1, the unit is 2^(e + 1 - 62) and the CAPACITY of a sum 2^(e + 1), at least twice the
 * bound.  A value converts exactly while it is a multiple of the unit, loses less than one unit otherwise (truncation) and contributes
 * nothing below 2^-23 units; a subnormal RESULT is outside the contract.
 * The contract, enforced: every value is +-0 or a positive finite number below the capacity, and every per-vertex sum stays below the
 * capacity.  A value that breaks it contributes nothing, the sums that it or an overflow touches are unspecified, and the call leaves a
 * VGL_HIP_SUM_* bit for vgl_hip_sum_over_edges_check.  The values of a gather block are checked when an edge reads from the block, the sums
 * in the epilogue.  Not detectable: a sum that wrapped past 2^64 units (more than four times the capacity) and came back below 2^62. */
int vgl_hip_sum_over_edges_f32(vgl_hip_ctx *ctx, vgl_hip_graph *g, const float *d_values, float sum_bound, float *d_sums);
#define VGL_HIP_SUM_NEGATIVE 1u        /* a value below zero (-0.0 is a zero) */
#define VGL_HIP_SUM_NOT_FINITE 2u      /* a NaN or an infinity */
#define VGL_HIP_SUM_VALUE_TOO_LARGE 4u /* a value at or above the capacity */
#define VGL_HIP_SUM_TOTAL_TOO_LARGE 8u /* a per-vertex sum at or above the capacity */
/* Waits for the context's stream; *violations = the VGL_HIP_SUM_* bits left by the vgl_hip_sum_over_edges_f32 calls on this context since
 * the last check (0: every one of them kept the contract), which are cleared.  Returns non-zero only when the check itself fails. */
int vgl_hip_sum_over_edges_check(vgl_hip_ctx *ctx, unsigned *violations);
int vgl_hip_pr_iteration_owned(vgl_hip_ctx *ctx, vgl_hip_graph *g, const int32_t *d_indeg_noloops, const float *d_rdeg,
                               float *d_ranks, float *d_contrib_scratch);
/* "Recently changed" exchange of a replicated 4-byte vertex array (EXCHANGE_RECENTLY_CHANGED, common/mpi_exchange.hpp:110-150): instead
 * of all-reducing V entries per super-step every rank sends the (index, value) pairs of the entries its step changed.
 * diff_to_pairs: d_out[0] = number of i < n with d_before[i] != d_after[i] (may exceed cap), then (index, value bits) pairs of the first
 * min(count, cap) of them, unordered; d_out holds 1 + 2 * cap int32.  Asynchronous.
 * apply_pairs: `parts` such lists, `stride` int32 apart; every pair is merged into d_values with min (take_min != 0: SSSP distances, CC
 * labels) or max (SSWP widths) on the 4-byte patterns (all values are non-negative); list `skip_part` (this rank's own, or -1) is
 * skipped.  changed (optional, synchronises): 1 if an entry of d_values moved. */
int vgl_hip_diff_to_pairs_u32(vgl_hip_ctx *ctx, int32_t n, const void *d_before, const void *d_after, int32_t cap, int32_t *d_out);
int vgl_hip_apply_pairs_u32(vgl_hip_ctx *ctx, int parts, int64_t stride, int skip_part, const int32_t *d_lists, int take_min, int32_t n,
                            void *d_values, int *changed);
/* in-degree without self loops from an out-CSR shard (adds into d_indeg; zero it first; allreduce(sum) across shards) */
int vgl_hip_indegree_noloops_add(vgl_hip_ctx *ctx, vgl_hip_graph *g, int32_t *d_indeg);

/* ---- multi-GPU behind the boundary: communicator, exchanges and the super-step loops (one process per GPU).
 *      Replaces GraphAbstractions::exchange_vertices_array (common/graph_abstractions.h:157-168) and its MPI implementation
 *      common/mpi_exchange.hpp:110-150 (EXCHANGE_RECENTLY_CHANGED), :156-187 (EXCHANGE_ALL with a merge operator), :222-271
 *      (EXCHANGE_PRIVATE_DATA); the library_data MPI rank / size of vgl_runtime/helpers/library_data/library_data.h.
 *      Transport RCCL: collectives over xGMI, enqueued on the context's stream -- kernels and collectives of a super-step are
 *      stream-ordered, the host waits only where it has to decide something (one pinned-memory poll per super-step).
 *      Transport HOSTED: the same collectives staged through a POSIX shared-memory segment; ranks are processes of one host and
 *      may share one GPU (RCCL refuses two ranks on one device) -- rehearsals and multi-rank tests on fewer GPUs than ranks. ---- */
typedef struct vgl_hip_comm vgl_hip_comm;
#define VGL_HIP_COMM_ID_BYTES 128
#define VGL_HIP_COMM_RCCL 0
#define VGL_HIP_COMM_HOSTED 1
#define VGL_HIP_COMM_PEER 2
/* rank 0 makes the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by any means (file, socket, MPI, torch store) */
int vgl_hip_comm_unique_id(void *id_out);
int vgl_hip_comm_create(vgl_hip_ctx *ctx, int rank, int world, const void *unique_id, vgl_hip_comm **out);
/* name: shared-memory object name common to the ranks ("/vgl_job42"); slot_bytes: staging capacity per rank (larger payloads go in pieces) */
int vgl_hip_comm_create_hosted(vgl_hip_ctx *ctx, int rank, int world, const char *name, size_t slot_bytes, vgl_hip_comm **out);
/* Transport PEER (round 4; what the reference hand-rolls with MPI point-to-point messages, vgl_compute_api/common/mpi_exchange.hpp:110-187,222-271):
 * every rank owns a window in device memory that the other ranks map (hipIpc; ranks = GPUs of one node over xGMI, or processes / threads
 * sharing one GPU) and write into from kernels on their own streams; arrival and consumption flags live in the windows; the exchanges of
 * a group share one flag round.  No collective library and no host in the data path.  name: shared-memory object used for the set-up
 * handshake only; window_bytes: capacity of one of the two halves of a window (larger payloads go in pieces).  Fails -- on every rank alike --
 * when a window cannot be mapped by a peer: fall back to vgl_hip_comm_create (RCCL). */
int vgl_hip_comm_create_peer(vgl_hip_ctx *ctx, int rank, int world, const char *name, size_t window_bytes, vgl_hip_comm **out);
/* bound of every in-kernel flag wait of the PEER transport from now on (ms; <= 0: the default, 20 s).  The variable VGL_PEER_TIMEOUT_MS is read once,
 * when the communicator is created; a caller that probes the transport with a short bound sets the working bound here afterwards.  Other transports: no-op. */
int vgl_hip_comm_set_timeout_ms(vgl_hip_comm *comm, double ms);
/* tells the other ranks of a hosted / peer communicator that this rank gives up: their next barrier fails at once instead of after its timeout */
int vgl_hip_comm_abort(vgl_hip_comm *comm);
int vgl_hip_comm_destroy(vgl_hip_comm *comm);
int vgl_hip_comm_info(vgl_hip_comm *comm, int *rank, int *world, int *transport);
int vgl_hip_comm_barrier(vgl_hip_comm *comm);            /* drains the stream, meets the other ranks */
/* EXCHANGE_ALL with the merge operators the algorithms use (shortest_paths.hpp:136-141 min_op; widest paths: max; pr.hpp:58 sum):
 * in-place all-reduce of a replicated device array, asynchronous on the context's stream */
int vgl_hip_exchange_allreduce_min_i32(vgl_hip_comm *comm, int32_t *d_values, int64_t n);
int vgl_hip_exchange_allreduce_min_f32(vgl_hip_comm *comm, float *d_values, int64_t n);
int vgl_hip_exchange_allreduce_max_f32(vgl_hip_comm *comm, float *d_values, int64_t n);
int vgl_hip_exchange_allreduce_sum_i32(vgl_hip_comm *comm, int32_t *d_values, int64_t n);
int vgl_hip_exchange_allreduce_sum_i64(vgl_hip_comm *comm, int64_t *d_values, int64_t n);
int vgl_hip_exchange_allreduce_sum_f32(vgl_hip_comm *comm, float *d_values, int64_t n);
int vgl_hip_exchange_allreduce_sum_f64(vgl_hip_comm *comm, double *d_values, int64_t n);
/* d_recv[p * bytes .. ) = rank p's d_send; asynchronous */
int vgl_hip_exchange_allgather(vgl_hip_comm *comm, const void *d_send, void *d_recv, int64_t bytes_per_rank);
/* EXCHANGE_PRIVATE_DATA (mpi_exchange.hpp:222-271, MPI_Allgatherv in place): rank p owns elements [bounds[p], bounds[p+1]) of the
 * replicated array (host array of world+1 entries, the same on every rank); afterwards every rank holds every owner's slice */
int vgl_hip_exchange_allgather_slices(vgl_hip_comm *comm, void *d_array, const int64_t *bounds_host, int elem_bytes);
/* every rank ends with the OR of all ranks' bitmaps (in place): all-to-all of the word slices, OR, all-gather -- 2 x words x 8 bytes per
 * rank instead of world x words x 8 */
int vgl_hip_exchange_bitmap_or(vgl_hip_comm *comm, uint64_t *d_bits, int64_t words);
/* EXCHANGE_RECENTLY_CHANGED in one call (diff -> counts -> lists -> merge; mpi_exchange.hpp:110-150): d_values is this rank's copy after its
 * super-step, d_before the copy before it; afterwards d_values holds the merge (min or max on the 4-byte patterns of non-negative values)
 * of every rank's changes.  One small all-gather when every rank changed at most 2048 entries (the counts ride in the payload), a second,
 * sized one otherwise, the whole-array all-reduce when some rank changed more than n / (2 world).  *changed_anywhere (synchronises): 1 if
 * any rank changed anything -- the loop condition of shortest_paths.hpp:143-152 without a flag reduction. */
int vgl_hip_exchange_changed_u32(vgl_hip_comm *comm, int32_t n, const void *d_before, void *d_values, int take_min, int *changed_anywhere);

/* The super-step loops over edge-cut shards (g owns rows [row_begin, row_end) of a graph of V vertices; vertex arrays are replicated,
 * V entries on every rank).  comm == NULL or a world of one: no exchange, same code path.  Results are bit-identical to the single-GPU
 * drivers (fixed points / owner-computed sums).
 *   bfs : direction-optimising (mode DIRECTION_OPT needs the incoming CSR of the owned rows and global_edges = E of the whole graph) or
 *         top-down; every rank must own a 64-aligned row range.  d_levels is complete on the OWNED rows when it returns; pass
 *         gather_levels != 0 to have the slices all-gathered (EXCHANGE_PRIVATE_DATA) so that every rank holds all levels.
 *   sssp / sswp : all-active push over the owned rows + changed-entries exchange (min / max)
 *   cc  : Shiloach-Vishkin hook over the owned rows + changed-entries exchange (min) + replicated pointer jumping
 *   pr  : owner-computes pull + all-gather of the owned slices; mode as vgl_hip_pr_run_mode, AUTO is resolved from the GLOBAL edge count
 *         and the GLOBAL longest row so that every rank takes the same path.  The in-degrees minus self loops of all vertices (pr.hpp:31-65)
 *         are counted and summed over the ranks on the first call with a graph handle and kept with it (the graph does not change) */
int vgl_hip_bfs_run_sharded(vgl_hip_ctx *ctx, vgl_hip_comm *comm, vgl_hip_graph *g, int32_t source, int mode, int64_t global_edges,
                            int gather_levels, int32_t *d_levels, vgl_hip_bfs_stats *stats);
int vgl_hip_sssp_run_sharded(vgl_hip_ctx *ctx, vgl_hip_comm *comm, vgl_hip_graph *g, const float *d_weights, int32_t source,
                             float *d_dist, vgl_hip_sssp_stats *stats);
int vgl_hip_sswp_run_sharded(vgl_hip_ctx *ctx, vgl_hip_comm *comm, vgl_hip_graph *g, const float *d_capacities, int32_t source,
                             float *d_widths, vgl_hip_sssp_stats *stats);
int vgl_hip_cc_run_sharded(vgl_hip_ctx *ctx, vgl_hip_comm *comm, vgl_hip_graph *g, int32_t *d_comp, vgl_hip_cc_stats *stats);
int vgl_hip_pr_run_sharded(vgl_hip_ctx *ctx, vgl_hip_comm *comm, vgl_hip_graph *g, int iterations, int mode, float *d_ranks,
                           vgl_hip_pr_stats *stats);
/* HITS over the shards (algorithms/hits/hits.hpp:32-91 with the exchanges at :52 and :79): replicated f64 authority / hub arrays, the owned
 * rows pulled per rank, one f64 all-reduce (sum of squares) and one all-gather of the owned slices per half step */
int vgl_hip_hits_run_sharded(vgl_hip_ctx *ctx, vgl_hip_comm *comm, vgl_hip_graph *g, int steps, double *d_auth, double *d_hub);
/* exchange statistics of the last *_run_sharded on this communicator: collectives issued, bytes this rank received, super-steps that
 * used pair lists / the whole-array all-reduce / id lists (BFS) */
typedef struct {
    int64_t collectives, bytes_received;
    int32_t list_steps, dense_steps, sparse_levels, exchanges;      /* exchanges: flag rounds of the PEER transport (the collectives of a group share one) */
} vgl_hip_exchange_stats;
int vgl_hip_comm_stats(vgl_hip_comm *comm, vgl_hip_exchange_stats *out);

/* ---- kernel timing hooks for bench.py's roofline line: when enabled every launch of the named dominant kernels
 *      is bracketed by hipEvents on the context stream; totals are read back afterwards. ---- */
int vgl_hip_timing_enable(vgl_hip_ctx *ctx, int enable);
/* restrict the bracketing to ONE kernel name (NULL or "" = all): two event records cost ~4-5 us of stream time per launch, which is
 * 10 % of a BFS traversal when every kernel is bracketed -- the timed region of bench.py brackets only the kernel it reports */
int vgl_hip_timing_only(vgl_hip_ctx *ctx, const char *kernel_name);
/* of the launches that would be bracketed only every stride-th is (1 = all): sampling instead of perturbing a launch-bound loop */
int vgl_hip_timing_stride(vgl_hip_ctx *ctx, int stride);
int vgl_hip_timing_reset(vgl_hip_ctx *ctx);
/* kernel_name: "bfs_bottom_up", "bfs_top_down", "gnf", "sssp_relax", "pr_pull", "cc_hook"; returns launches and total ms */
int vgl_hip_timing_get(vgl_hip_ctx *ctx, const char *kernel_name, int64_t *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif
