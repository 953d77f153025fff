"""Host-side harness over the C ABI (include/vgl_hip.h): graph construction, frontier objects and the
fused BFS / SSSP / PageRank / CC entry points, with torch tensors used only as device-memory handles
(pointers and sizes cross the boundary; no torch types do).

Names follow the reference: VGL_Graph -> Graph (outgoing + incoming CSR, vgl_graph.h:7-79),
VGL_Frontier -> Frontier (base_frontier.h:5-62), algorithms/{bfs,sssp,pr,cc} -> bfs(), sssp(), page_rank(),
connected_components().  The C++ drop-in class for arbitrary user lambdas is
vectorgraphlibrary_amd/hip/vgl_hip.hpp.
"""
import ctypes as C

import torch

from . import lib as _l

RMAT_ABCD = (57, 19, 19, 5)            # vgl_runtime.hpp:36
BFS_TOP_DOWN, BFS_DIRECTION_OPT = 0, 1
SSSP_ALL_ACTIVE, SSSP_ACTIVE_TILES, SSSP_DELTA_STEPPING, SSSP_PULL, SSSP_DIRECTION_OPT = 0, 1, 2, 3, 4
DENSE, SPARSE, ALL_ACTIVE = 0, 1, 2    # framework_types.h:156-160
PR_EXACT_ORDER, PR_BLOCKED, PR_AUTO = 0, 1, 2
# VGL_HIP_SUM_* of include/vgl_hip.h: what vgl_hip_sum_over_edges_check reports
SUM_VIOLATIONS = ((1, "negative value"), (2, "value not finite"), (4, "value at or above the capacity"), (8, "sum at or above the capacity"))
LP_ALL_ACTIVE, LP_FRONTIER, LP_AUTO = 0, 1, 2


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Context:
    """One per GPU / process.  Work is ordered on torch's current stream of `device` so that it composes
    with torch.distributed (RCCL) collectives issued from the same process."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise _l.VglHipError("no HIP device visible: vectorgraphlibrary_amd has no CPU fallback")
        self.L = _l.load()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        h = C.c_void_p()
        _l.check(self.L.vgl_hip_ctx_create(device, C.c_void_p(stream), C.byref(h)))
        self.h = h

    def sync(self):
        _l.check(self.L.vgl_hip_ctx_sync(self.h))

    def close(self):
        if self.h:
            self.L.vgl_hip_ctx_destroy(self.h)
            self.h = None

    def empty(self, n, dtype):
        return torch.empty(int(n), dtype=dtype, device=self.device)

    # ---- timing hooks (bench.py roofline) ----
    def timing(self, enable=True, only=None, stride=1):
        """bracket kernel launches with HIP events (only: one kernel name; the rest then run without the event records; stride: only every
        stride-th of the bracketed launches)"""
        _l.check(self.L.vgl_hip_timing_enable(self.h, int(enable)))
        _l.check(self.L.vgl_hip_timing_only(self.h, only.encode() if only else None))
        _l.check(self.L.vgl_hip_timing_stride(self.h, int(stride)))
        _l.check(self.L.vgl_hip_timing_reset(self.h))

    def timing_get(self, name):
        n, ms = C.c_int64(), C.c_double()
        _l.check(self.L.vgl_hip_timing_get(self.h, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def bfs_front_fold(self, front, words=None):
        """vgl_hip_bfs_front_fold: the first `words` 64-bit words of the frontier bitmap `front` (int64 tensor) folded onto 2048 words, as the
        filtered bottom-up probe of bfs() reads it"""
        words = front.numel() if words is None else int(words)
        fold = self.empty(2048, torch.int64)
        _l.check(self.L.vgl_hip_bfs_front_fold(self.h, words, _ptr(front), _ptr(fold)))
        return fold

    # ---- synthetic inputs ----
    def gen_rmat(self, scale, edge_factor, seed, relabel=True, first_edge=0, count=None):
        E = (1 << scale) * edge_factor if count is None else count
        src, dst = self.empty(E, torch.int32), self.empty(E, torch.int32)
        a, b, c, d = RMAT_ABCD
        _l.check(self.L.vgl_hip_gen_rmat(self.h, scale, first_edge, E, seed, a, b, c, d, int(relabel), _ptr(src), _ptr(dst)))
        return src, dst

    def gen_uniform(self, scale, edge_factor, seed, first_edge=0, count=None):
        E = (1 << scale) * edge_factor if count is None else count
        src, dst = self.empty(E, torch.int32), self.empty(E, torch.int32)
        _l.check(self.L.vgl_hip_gen_uniform(self.h, scale, first_edge, E, seed, _ptr(src), _ptr(dst)))
        return src, dst

    def gen_weights(self, E, seed, first_edge=0):
        w = self.empty(E, torch.float32)
        _l.check(self.L.vgl_hip_gen_weights(self.h, first_edge, E, seed, _ptr(w)))
        return w

    def coo_to_csr(self, V, src, dst, row_begin=0, row_end=None, want_perm=False):
        """stable COO -> CSR of the edges whose source lies in [row_begin,row_end)."""
        row_end = V if row_end is None else row_end
        E = src.numel()
        rowptr = self.empty(row_end - row_begin + 1, torch.int64)
        adj = self.empty(max(E, 1), torch.int32)
        perm = self.empty(max(E, 1), torch.int64) if want_perm else None
        kept = C.c_int64()
        _l.check(self.L.vgl_hip_coo_to_csr(self.h, V, E, _ptr(src), _ptr(dst), row_begin, row_end, _ptr(rowptr), _ptr(adj),
                                           _ptr(perm), C.byref(kept)))
        k = kept.value
        return rowptr, adj[:k], (perm[:k] if want_perm else None)

    def gather_u32(self, perm, values):
        out = torch.empty(perm.numel(), dtype=values.dtype, device=self.device)
        _l.check(self.L.vgl_hip_gather_u32(self.h, perm.numel(), _ptr(perm), _ptr(values), _ptr(out)))
        return out

    def degree_order(self, V, src, dst, kind="total"):
        """VectCSR-style renumbering: fwd[orig] = sorted id, bwd[sorted] = orig (degree descending, id ascending)."""
        fwd, bwd = self.empty(V, torch.int32), self.empty(V, torch.int32)
        k = {"out": 0, "in": 1, "total": 2}[kind]
        _l.check(self.L.vgl_hip_degree_order(self.h, V, src.numel(), _ptr(src), _ptr(dst), k, _ptr(fwd), _ptr(bwd)))
        return fwd, bwd

    def degree_hist_add(self, src, dst, kind, degree):
        """degree[v] += degree of v in the chunk (src,dst); degree is a zero-initialised 4-byte vertex array"""
        k = {"out": 0, "in": 1, "total": 2}[kind]
        _l.check(self.L.vgl_hip_degree_hist_add(self.h, src.numel(), _ptr(src), _ptr(dst), k, _ptr(degree)))

    def degree_order_from_degrees(self, degree):
        V = degree.numel()
        fwd, bwd = self.empty(V, torch.int32), self.empty(V, torch.int32)
        _l.check(self.L.vgl_hip_degree_order_from_degrees(self.h, V, _ptr(degree), _ptr(fwd), _ptr(bwd)))
        return fwd, bwd

    def relabel(self, mapping, ids):
        out = torch.empty_like(ids)
        _l.check(self.L.vgl_hip_relabel_i32(self.h, ids.numel(), _ptr(mapping), _ptr(ids), _ptr(out)))
        return out

    def permute(self, idx, values):
        """out[i] = values[idx[i]] for a 4-byte vertex array"""
        out = torch.empty_like(values)
        _l.check(self.L.vgl_hip_permute_u32(self.h, values.numel(), _ptr(idx), _ptr(values), _ptr(out)))
        return out

    def partition_rows(self, rowptr, parts):
        V = rowptr.numel() - 1
        bounds = (C.c_int32 * (parts + 1))()
        _l.check(self.L.vgl_hip_partition_rows(self.h, V, _ptr(rowptr), parts, bounds))
        return list(bounds)


class Graph:
    """Device CSR in both directions (or outgoing only), optionally restricted to the owned rows [row_begin,row_end)."""

    def __init__(self, ctx, V, out_rowptr, out_adj, in_rowptr=None, in_adj=None, row_begin=0, row_end=None):
        self.ctx, self.V = ctx, int(V)
        self.row_begin, self.row_end = int(row_begin), int(V if row_end is None else row_end)
        self.out_rowptr, self.out_adj, self.in_rowptr, self.in_adj = out_rowptr, out_adj, in_rowptr, in_adj
        self.E = int(out_adj.numel())
        self.fwd = self.bwd = None            # set by from_coo(renumber=...): original <-> sorted vertex ids
        self.perm = None
        h = C.c_void_p()
        _l.check(ctx.L.vgl_hip_graph_create(ctx.h, self.V, self.row_begin, self.row_end, _ptr(out_rowptr), _ptr(out_adj), self.E,
                                            _ptr(in_rowptr), _ptr(in_adj), int(in_adj.numel()) if in_adj is not None else 0,
                                            C.byref(h)))
        self.h = h

    @classmethod
    def from_coo(cls, ctx, V, src, dst, with_incoming=True, want_perm=False, renumber=None):
        """VGL_Graph::import (vgl_graph.hpp:57-68): outgoing CSR from (src,dst), incoming CSR from the OUT-CSR-ordered
        transposed list (the container is sorted in place by the outgoing import before it is transposed).
        renumber in {None, "out", "in", "total"}: VectCSR-style degree renumbering of the vertices before the build
        (vect_csr/import.hpp:61-99); vertex arrays of such a graph live in the sorted numbering (see to_original)."""
        fwd = bwd = None
        if renumber:
            fwd, bwd = ctx.degree_order(V, src, dst, renumber)
            src, dst = ctx.relabel(fwd, src), ctx.relabel(fwd, dst)
        rowptr, adj, perm = ctx.coo_to_csr(V, src, dst, want_perm=want_perm)
        in_rowptr = in_adj = None
        if with_incoming:
            deg = rowptr[1:] - rowptr[:-1]
            csr_src = torch.repeat_interleave(torch.arange(V, device=ctx.device, dtype=torch.int32), deg)
            in_rowptr, in_adj, _ = ctx.coo_to_csr(V, adj, csr_src)
            del csr_src
        g = cls(ctx, V, rowptr, adj, in_rowptr, in_adj)
        g.perm, g.fwd, g.bwd = perm, fwd, bwd
        return g

    def vertex_id(self, original_id):
        """original vertex id -> id in this graph's numbering (VGL_Graph::reorder(v, ORIGINAL, SCATTER))"""
        return int(self.fwd[original_id]) if self.fwd is not None else int(original_id)

    def to_original(self, values):
        """vertex array in this graph's numbering -> ORIGINAL numbering (VerticesArray::reorder(ORIGINAL))"""
        return self.ctx.permute(self.fwd, values) if self.fwd is not None else values

    def shard(self, row_begin, row_end):
        """edge-cut shard owning rows [row_begin,row_end) of both directions (own, aligned copies of the slices)."""
        def cut(rowptr, adj):
            if rowptr is None:
                return None, None
            lo, hi = int(rowptr[row_begin]), int(rowptr[row_end])
            return (rowptr[row_begin:row_end + 1] - lo).contiguous(), adj[lo:hi].clone()
        orp, oadj = cut(self.out_rowptr, self.out_adj)
        irp, iadj = cut(self.in_rowptr, self.in_adj)
        s = Graph(self.ctx, self.V, orp, oadj, irp, iadj, row_begin, row_end)
        s.fwd, s.bwd = self.fwd, self.bwd
        return s

    def info(self):
        """what creation derived for the BFS (vgl_hip_graph_info): rows with incoming edges, the form of their head records, and reach_rows =
        1 + the largest owned vertex with an incoming edge (0: none; V without the incoming CSR), below which a traversal's writes stay"""
        n, p, r = C.c_int32(), C.c_int(), C.c_int32()
        _l.check(self.ctx.L.vgl_hip_graph_info(self.h, C.byref(n), C.byref(p), C.byref(r)))
        return {"in_nz_rows": n.value, "bfs_heads": "packed" if p.value else "wide", "reach_rows": r.value}

    def out_edge_range(self, row_begin, row_end):
        return int(self.out_rowptr[row_begin]), int(self.out_rowptr[row_end])

    def prepare_page_rank(self, mode=PR_AUTO):
        """build now what the first page_rank() call would build (blocked layout or hub schedule); returns the resolved mode"""
        m = C.c_int()
        _l.check(self.ctx.L.vgl_hip_pr_prepare(self.ctx.h, self.h, int(mode), C.byref(m)))
        return m.value

    def prepare_sssp(self):
        """build the blocked STRUCTURE of the path algorithms now (once per graph; vgl_hip_sssp_prepare): afterwards a pull plan for any weights
        array is one gather pass and SSSP_ALL_ACTIVE runs as blocked passes"""
        _l.check(self.ctx.L.vgl_hip_sssp_prepare(self.ctx.h, self.h))

    def prepare_cc(self):
        _l.check(self.ctx.L.vgl_hip_cc_prepare(self.ctx.h, self.h))

    def prepare_label_propagation(self, direction="out"):
        """degree classes of `direction` (and the push schedule of its reverse) now, outside any timing (vgl_hip_lp_prepare)"""
        _l.check(self.ctx.L.vgl_hip_lp_prepare(self.ctx.h, self.h, {"out": 0, "in": 1}[direction]))

    def prepare_triangle_count(self):
        """the oriented CSR and row classes of triangle_count() now, outside any timing (vgl_hip_tri_prepare)"""
        _l.check(self.ctx.L.vgl_hip_tri_prepare(self.ctx.h, self.h))

    def prepare_betweenness(self, symmetric=False):
        """the row classes of betweenness_centrality() now, outside any timing (vgl_hip_bc_prepare)"""
        _l.check(self.ctx.L.vgl_hip_bc_prepare(self.ctx.h, self.h, int(bool(symmetric))))

    def prepare_msbfs(self, direction="out", symmetric=False):
        """the row classes of multi_source_bfs() (and of closeness_centrality(), harmonic_centrality(), eccentricity()) for `direction` now, outside
        any timing (vgl_hip_msbfs_prepare)"""
        _l.check(self.ctx.L.vgl_hip_msbfs_prepare(self.ctx.h, self.h, {"out": 0, "in": 1}[direction], int(bool(symmetric))))

    def prepare_ppr(self, symmetric=False):
        """the sorted row-class lists and the chunk table of personalized_pagerank() / pagerank() now, outside any timing (vgl_hip_ppr_prepare)"""
        _l.check(self.ctx.L.vgl_hip_ppr_prepare(self.ctx.h, self.h, int(bool(symmetric))))

    def prepare_kcore(self):
        """the symmetric simple CSR of core_numbers() / k_core() now, outside any timing (vgl_hip_kcore_prepare)"""
        _l.check(self.ctx.L.vgl_hip_kcore_prepare(self.ctx.h, self.h))

    def prepare_ktruss(self):
        """the edge numbering of truss_numbers() / k_truss() (and the symmetric simple CSR it shares with core_numbers()) now, outside any timing
        (vgl_hip_ktruss_prepare); returns the number of undirected edges"""
        n = C.c_int64()
        _l.check(self.ctx.L.vgl_hip_ktruss_prepare(self.ctx.h, self.h, C.byref(n)))
        return n.value

    def prepare_msf(self):
        """what minimum_spanning_forest() keeps per graph (the symmetric simple CSR, the edge numbering it shares with truss_numbers() and the edge of
        every stored entry) now, outside any timing (vgl_hip_msf_prepare); returns the number of undirected edges"""
        n = C.c_int64()
        _l.check(self.ctx.L.vgl_hip_msf_prepare(self.ctx.h, self.h, C.byref(n)))
        return n.value

    def prepare_bicc(self):
        """the edge numbering of biconnected_components() / bridges() (and the symmetric simple CSR it shares with core_numbers()) now, outside any
        timing (vgl_hip_bicc_prepare); returns the number of undirected edges"""
        n = C.c_int64()
        _l.check(self.ctx.L.vgl_hip_bicc_prepare(self.ctx.h, self.h, C.byref(n)))
        return n.value

    def prepare_mis(self):
        """the symmetric simple CSR of maximal_independent_set() (shared with core_numbers()) now, outside any timing (vgl_hip_mis_prepare)"""
        _l.check(self.ctx.L.vgl_hip_mis_prepare(self.ctx.h, self.h))

    def prepare_matching(self):
        """the edge numbering of maximal_matching() / vertex_cover() (shared with truss_numbers(), minimum_spanning_forest() and
        biconnected_components()) now, outside any timing (vgl_hip_matching_prepare); returns the number of undirected edges"""
        n = C.c_int64()
        _l.check(self.ctx.L.vgl_hip_matching_prepare(self.ctx.h, self.h, C.byref(n)))
        return n.value

    def prepare_similarity(self):
        """the symmetric simple CSR (shared with core_numbers()) and the 2-path counts of common_neighbors() / similarity() / link_prediction() now,
        outside any timing (vgl_hip_sim_prepare)"""
        _l.check(self.ctx.L.vgl_hip_sim_prepare(self.ctx.h, self.h))

    def prepare_blocked_bfs(self):
        """one-time layout for the blocked top-down BFS levels (vgl_hip_bfs_prepare_blocked); bfs() results do not change"""
        _l.check(self.ctx.L.vgl_hip_bfs_prepare_blocked(self.ctx.h, self.h))

    def close(self):
        for plan in self.__dict__.pop("_agg_plans", {}).values():      # the plans of aggregate_neighbors borrow this graph's arrays
            plan.close()
        if self.h:
            self.ctx.L.vgl_hip_graph_destroy(self.ctx.h, self.h)
            self.h = None


class Frontier:
    def __init__(self, graph):
        self.g, self.ctx = graph, graph.ctx
        h = C.c_void_p()
        _l.check(self.ctx.L.vgl_hip_frontier_create(self.ctx.h, graph.h, C.byref(h)))
        self.h = h

    def set_all_active(self):
        _l.check(self.ctx.L.vgl_hip_frontier_set_all_active(self.ctx.h, self.h))

    def clear(self):
        _l.check(self.ctx.L.vgl_hip_frontier_clear(self.ctx.h, self.h))

    def add_vertex(self, v):
        _l.check(self.ctx.L.vgl_hip_frontier_add_vertex(self.ctx.h, self.h, int(v)))

    def info(self):
        s, n, t = C.c_int32(), C.c_int64(), C.c_int()
        _l.check(self.ctx.L.vgl_hip_frontier_info(self.ctx.h, self.h, C.byref(s), C.byref(n), C.byref(t)))
        return s.value, n.value, t.value

    def size(self):
        return self.info()[0]

    def _view(self, ptr, n):
        if n == 0:
            return torch.empty(0, dtype=torch.int32)
        buf = torch.empty(n, dtype=torch.int32)
        _l.check(self.ctx.L.vgl_hip_memcpy_d2h(self.ctx.h, C.c_void_p(buf.data_ptr()), C.c_void_p(ptr), n * 4))
        return buf

    def ids(self):
        return self._view(self.ctx.L.vgl_hip_frontier_ids(self.h), self.size())

    def flags(self):
        return self._view(self.ctx.L.vgl_hip_frontier_flags(self.h), self.g.V)

    def generate_from_flags(self, flags, dense_threshold=0.0):
        _l.check(self.ctx.L.vgl_hip_gnf_from_flags(self.ctx.h, self.g.h, _ptr(flags), float(dense_threshold), self.h))

    def generate_equal(self, values, value, dense_threshold=0.0):
        _l.check(self.ctx.L.vgl_hip_gnf_equal_i32(self.ctx.h, self.g.h, _ptr(values), int(value), float(dense_threshold), self.h))

    def reduce_sum(self, values):
        if values.dtype == torch.int32:
            r = C.c_int64()
            _l.check(self.ctx.L.vgl_hip_reduce_sum_i32(self.ctx.h, self.h, _ptr(values), C.byref(r)))
        else:
            r = C.c_double()
            _l.check(self.ctx.L.vgl_hip_reduce_sum_f32(self.ctx.h, self.h, _ptr(values), C.byref(r)))
        return r.value

    def close(self):
        if self.h:
            self.ctx.L.vgl_hip_frontier_destroy(self.ctx.h, self.h)
            self.h = None


def _stats(s):
    return {k: getattr(s, k) for k, _ in s._fields_}


# The entry points below take the source in ORIGINAL vertex ids and, by default, return the result in ORIGINAL
# numbering.  raw=True skips both conversions (source and result in the graph's own numbering): that is the timed region
# of the reference, which reorders before tm.start() and after tm.end() (bfs.hpp:62-85, verify_results.h:33-92).

def bfs(graph, source, mode=BFS_DIRECTION_OPT, levels=None, raw=False):
    ctx = graph.ctx
    levels = ctx.empty(graph.V, torch.int32) if levels is None else levels
    st = _l.BfsStats()
    s = int(source) if raw else graph.vertex_id(source)
    _l.check(ctx.L.vgl_hip_bfs_run(ctx.h, graph.h, s, mode, _ptr(levels), C.byref(st)))
    return (levels if raw else graph.to_original(levels)), _stats(st)


def bfs_batch(graph, sources, mode=BFS_DIRECTION_OPT, levels=None):
    """vgl_hip_bfs_run_batch: the traversals from `sources` (the graph's own numbering) one after the other behind ONE call of the C ABI -- the rounds
    loop of the reference's bfs app; returns (levels of the last source, list of per-traversal stats)."""
    ctx = graph.ctx
    levels = ctx.empty(graph.V, torch.int32) if levels is None else levels
    n = len(sources)
    src = (C.c_int32 * n)(*[int(s) for s in sources])
    st = (_l.BfsStats * n)()
    _l.check(ctx.L.vgl_hip_bfs_run_batch(ctx.h, graph.h, src, n, mode, _ptr(levels), st))
    return levels, [_stats(st[i]) for i in range(n)]


class SsspPlan:
    """light/heavy partitioned copy of (adjacency, weights) for the bucketed SSSP schedule; reusable across sources."""

    def __init__(self, graph, weights, delta):
        self.g, self.ctx, self.delta = graph, graph.ctx, float(delta)
        h = C.c_void_p()
        _l.check(self.ctx.L.vgl_hip_sssp_plan_create(self.ctx.h, graph.h, _ptr(weights), self.delta, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            self.ctx.L.vgl_hip_sssp_plan_destroy(self.ctx.h, self.h)
            self.h = None


class SsspPullPlan:
    """blocked copy of (outgoing adjacency, edge values) for the pull steps of SSSP / SSWP (vgl_blocked.h); reusable across sources."""

    def __init__(self, graph, weights):
        self.g, self.ctx, self.weights = graph, graph.ctx, weights
        h = C.c_void_p()
        _l.check(self.ctx.L.vgl_hip_sssp_pull_plan_create(self.ctx.h, graph.h, _ptr(weights), C.byref(h)))
        self.h = h

    def info(self):
        e, f, b, m = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _l.check(self.ctx.L.vgl_hip_sssp_pull_plan_info(self.h, C.byref(e), C.byref(f), C.byref(b), C.byref(m)))
        return {"edges": e.value, "fused_edges": f.value, "streamed_bytes_per_pass": b.value, "plan_bytes": m.value}

    def close(self):
        if self.h:
            self.ctx.L.vgl_hip_sssp_pull_plan_destroy(self.ctx.h, self.h)
            self.h = None


def sssp(graph, weights, source, mode=SSSP_ACTIVE_TILES, dist=None, raw=False, delta=16.0, plan=None):
    """mode: SSSP_ALL_ACTIVE / SSSP_ACTIVE_TILES (push), SSSP_DELTA_STEPPING, SSSP_PULL, SSSP_DIRECTION_OPT (push <-> pull).
    plan: an SsspPlan (bucketed schedule) or an SsspPullPlan (with mode SSSP_PULL or SSSP_DIRECTION_OPT)."""
    ctx = graph.ctx
    dist = ctx.empty(graph.V, torch.float32) if dist is None else dist
    st = _l.SsspStats()
    s = int(source) if raw else graph.vertex_id(source)
    if isinstance(plan, SsspPullPlan):
        m = mode if mode in (SSSP_PULL, SSSP_DIRECTION_OPT) else SSSP_DIRECTION_OPT
        _l.check(ctx.L.vgl_hip_sssp_run_pull(ctx.h, graph.h, _ptr(weights), plan.h, s, int(m), _ptr(dist), C.byref(st)))
    elif plan is not None:
        _l.check(ctx.L.vgl_hip_sssp_run_plan(ctx.h, graph.h, plan.h, s, _ptr(dist), C.byref(st)))
    elif mode == SSSP_DELTA_STEPPING:
        _l.check(ctx.L.vgl_hip_sssp_run_delta(ctx.h, graph.h, _ptr(weights), s, float(delta), _ptr(dist), C.byref(st)))
    else:
        _l.check(ctx.L.vgl_hip_sssp_run(ctx.h, graph.h, _ptr(weights), s, mode, _ptr(dist), C.byref(st)))
    return (dist if raw else graph.to_original(dist)), _stats(st)


def sswp(graph, capacities, source, mode=SSSP_ACTIVE_TILES, widths=None, raw=False, plan=None):
    """single-source widest paths (SSWP::vgl_dijkstra): widths[source] = FLT_MAX, unreachable vertices 0; capacities in the
    order of the outgoing CSR.  source / result in ORIGINAL numbering unless raw=True."""
    ctx = graph.ctx
    widths = ctx.empty(graph.V, torch.float32) if widths is None else widths
    st = _l.SsspStats()
    src = int(source) if raw else graph.vertex_id(source)
    if isinstance(plan, SsspPullPlan):
        m = mode if mode in (SSSP_PULL, SSSP_DIRECTION_OPT) else SSSP_DIRECTION_OPT
        _l.check(ctx.L.vgl_hip_sswp_run_pull(ctx.h, graph.h, _ptr(capacities), plan.h, src, int(m), _ptr(widths), C.byref(st)))
    else:
        _l.check(ctx.L.vgl_hip_sswp_run(ctx.h, graph.h, _ptr(capacities), src, int(mode), _ptr(widths), C.byref(st)))
    return (widths if raw else graph.to_original(widths)), _stats(st)


def page_rank(graph, iterations, indeg_noloops=None, ranks=None, raw=False, mode=PR_AUTO):
    """indeg_noloops (optional) is indexed in the graph's own numbering.  mode: PR_EXACT_ORDER (adjacency-order f32 sums, bit-identical
    to seq_page_rank), PR_BLOCKED (LDS-window gather / sum, within a few ulp) or PR_AUTO (blocked from 2^25 edges)."""
    ctx = graph.ctx
    ranks = ctx.empty(graph.V, torch.float32) if ranks is None else ranks
    st = _l.PrStats()
    _l.check(ctx.L.vgl_hip_pr_run_mode(ctx.h, graph.h, _ptr(indeg_noloops), int(iterations), int(mode), _ptr(ranks), C.byref(st)))
    return (ranks if raw else graph.to_original(ranks)), _stats(st)


def sum_over_edges(graph, values, bound=1.0):
    """sums[src] = sum of values[dst] over the edges src -> dst with dst != src (graph's own numbering; the declared operator VGL_SUM_OVER_EDGES):
    exact fixed-point sums rounded to f32 once.  values: non-negative finite f32 (-0.0 is a zero), every per-vertex sum at most `bound`.
    Raises VglHipError naming what broke that contract (include/vgl_hip.h: the capacity of a value and of a sum is a power of two, at
    least twice the bound); a sum that wrapped past four times the capacity cannot be detected."""
    ctx = graph.ctx
    sums = ctx.empty(graph.V, torch.float32)
    _l.check(ctx.L.vgl_hip_sum_over_edges_f32(ctx.h, graph.h, _ptr(values), C.c_float(float(bound)), _ptr(sums)))
    bits = C.c_uint(0)
    _l.check(ctx.L.vgl_hip_sum_over_edges_check(ctx.h, C.byref(bits)))      # waits for the stream
    if bits.value:
        kinds = [name for bit, name in SUM_VIOLATIONS if bits.value & bit]
        raise _l.VglHipError("sum_over_edges: " + ", ".join(kinds) + f" (bound {float(bound)!r})")
    return sums


def strongly_connected_components(graph, raw=False):
    """labels = smallest ORIGINAL vertex id of each strongly connected component (raw=True: smallest id in the graph's numbering)"""
    ctx = graph.ctx
    comp = ctx.empty(graph.V, torch.int32)
    st = _l.SccStats()
    _l.check(ctx.L.vgl_hip_scc_run(ctx.h, graph.h, _ptr(comp), C.byref(st)))
    if raw or graph.fwd is None:
        return comp, _stats(st)
    out, scratch = ctx.empty(graph.V, torch.int32), ctx.empty(graph.V, torch.int32)
    _l.check(ctx.L.vgl_hip_cc_labels_to_original(ctx.h, graph.V, _ptr(comp), _ptr(graph.fwd), _ptr(graph.bwd), _ptr(scratch), _ptr(out)))
    return out, _stats(st)


def hits(graph, steps, raw=False):
    """HITS authorities and hubs (f64) after `steps` steps; needs the incoming CSR.  ORIGINAL numbering unless raw=True."""
    ctx = graph.ctx
    auth, hub = ctx.empty(graph.V, torch.float64), ctx.empty(graph.V, torch.float64)
    _l.check(ctx.L.vgl_hip_hits_run(ctx.h, graph.h, int(steps), _ptr(auth), _ptr(hub)))
    if raw or graph.fwd is None:
        return auth, hub
    idx = graph.fwd.long()
    return auth[idx], hub[idx]


def connected_components(graph, comp=None, raw=False, symmetric=False):
    """labels = smallest ORIGINAL vertex id that reaches each vertex (raw=True: smallest id in the graph's numbering).
    On a DIRECTED graph the hook / jump fixed point ("smallest id that reaches v") depends on the vertex numbering -- as in the
    reference (exact under identical numbering) -- so with a renumbered graph the conversion back to original ids is
    only meaningful for symmetric inputs, where the labels describe the components.
    symmetric=True: the caller vouches that every edge is stored in both directions; the same labels then come from a min-id
    union-find (vgl_hip_cc_run_symmetric) instead of repeated sweeps over all edges."""
    ctx = graph.ctx
    comp = ctx.empty(graph.V, torch.int32) if comp is None else comp
    st = _l.CcStats()
    run = ctx.L.vgl_hip_cc_run_symmetric if symmetric else ctx.L.vgl_hip_cc_run
    _l.check(run(ctx.h, graph.h, _ptr(comp), C.byref(st)))
    if raw or graph.fwd is None:
        return comp, _stats(st)
    out, scratch = ctx.empty(graph.V, torch.int32), ctx.empty(graph.V, torch.int32)
    _l.check(ctx.L.vgl_hip_cc_labels_to_original(ctx.h, graph.V, _ptr(comp), _ptr(graph.fwd), _ptr(graph.bwd), _ptr(scratch), _ptr(out)))
    return out, _stats(st)


def label_propagation(graph, max_iterations=20, direction="out", mode=LP_AUTO, labels=None, symmetric=False, raw=False):
    """label propagation (the contract of vgl_hip_lp_run in include/vgl_hip.h): every iteration each vertex takes the most frequent label among
    its neighbours in `direction` ("out" / "in"), ties to the largest label, until nothing changes or after max_iterations.
    labels: int32 start labels in ORIGINAL vertex order (raw=True: the graph's own order); None = the original vertex ids.
    mode: LP_ALL_ACTIVE, LP_FRONTIER or LP_AUTO (same answer).  symmetric=True: the caller vouches that every edge is stored both ways.
    Returns (labels in ORIGINAL order unless raw=True, stats dict with "changed_history")."""
    ctx = graph.ctx
    if labels is not None:
        labels = torch.as_tensor(labels, dtype=torch.int32, device=ctx.device).contiguous()
        init = labels if (raw or graph.fwd is None) else ctx.permute(graph.bwd, labels)
    else:
        init = graph.bwd                      # None for a graph in original numbering: the library starts from the ids
    out = ctx.empty(graph.V, torch.int32)
    hist = (C.c_int64 * max(int(max_iterations), 1))()
    st = _l.LpStats()
    _l.check(ctx.L.vgl_hip_lp_run(ctx.h, graph.h, {"out": 0, "in": 1}[direction], int(mode), int(bool(symmetric)), int(max_iterations),
                                  _ptr(init), _ptr(out), hist, C.byref(st)))
    stats = _stats(st)
    stats["changed_history"] = [hist[i] for i in range(st.iterations)]
    return (out if raw else graph.to_original(out)), stats


def triangle_count(graph, per_vertex=False, clustering=False, raw=False):
    """triangles of the simple undirected graph underlying the stored outgoing CSR (the contract of vgl_hip_tri_run in include/vgl_hip.h; `tc` is
    transitive closure, this is `tri`).  Returns (triangles, stats dict).  per_vertex=True adds stats["per_vertex"] (int64 tensor: triangles that
    contain each vertex); clustering=True adds that, stats["degree"] (int32, undirected simple degree) and stats["clustering"] (float64:
    2 t / (d (d - 1)), 0 where d < 2) -- all in ORIGINAL vertex order unless raw=True."""
    ctx = graph.ctx
    want_pv = bool(per_vertex or clustering)
    pv = ctx.empty(graph.V, torch.int64) if want_pv else None
    deg = ctx.empty(graph.V, torch.int32) if clustering else None
    tri = C.c_int64()
    st = _l.TriStats()
    _l.check(ctx.L.vgl_hip_tri_run(ctx.h, graph.h, C.byref(tri), _ptr(pv), _ptr(deg), C.byref(st)))
    stats = _stats(st)
    if want_pv:
        # 8-byte values: reordered with a torch index over the same mapping that to_original applies to 4-byte arrays
        stats["per_vertex"] = pv if (raw or graph.fwd is None) else pv[graph.fwd.long()]
    if clustering:
        deg = deg if raw else graph.to_original(deg)
        d = deg.to(torch.float64)
        pairs = d * (d - 1.0)
        stats["degree"] = deg
        stats["clustering"] = torch.where(deg >= 2, 2.0 * stats["per_vertex"].to(torch.float64) / torch.clamp(pairs, min=1.0), torch.zeros_like(d))
    return int(tri.value), stats


def betweenness_centrality(graph, sources=None, symmetric=False, rescale=False, halve=False, raw=False, want_last=False, bc=None):
    """betweenness centrality of the stored directed graph (the contract of vgl_hip_bc_run in include/vgl_hip.h): bc[v] = sum over the sources
    s != v of Brandes' dependency delta_s[v]; float64, unnormalised, endpoints not counted, multi-edges with their multiplicity.
    sources: None = every vertex (exact), else a sequence / tensor of ORIGINAL vertex ids (raw=True: the graph's own ids).  symmetric=True: the caller
    vouches that every edge is stored both ways (no incoming CSR needed).  rescale multiplies by V / len(sources), halve by 1/2 (an undirected graph
    stored both ways counts every pair twice).  bc: a float64 tensor in the graph's OWN numbering to accumulate into (implies raw; no rescale / halve).
    want_last adds the last source's "levels", "sigma", "delta".  Returns (bc in ORIGINAL order unless raw=True, stats dict)."""
    ctx = graph.ctx
    V = graph.V
    if sources is None:
        ids = list(range(V))
    else:
        ids = [int(s) for s in (sources.tolist() if torch.is_tensor(sources) else sources)]
    if not raw and bc is None and graph.fwd is not None and ids:
        if min(ids) < 0 or max(ids) >= V:
            raise _l.VglHipError("betweenness_centrality: source vertex out of range")
        fwd = graph.fwd.cpu()
        ids = [int(fwd[s]) for s in ids]
    n = len(ids)
    src = (C.c_int32 * max(n, 1))(*ids)
    accumulate = bc is not None
    if accumulate and (rescale or halve):
        raise _l.VglHipError("betweenness_centrality: rescale / halve do not apply to an accumulating call")
    out = bc if accumulate else ctx.empty(V, torch.float64)
    levels = ctx.empty(V, torch.int32) if want_last else None
    sigma = ctx.empty(V, torch.float64) if want_last else None
    delta = ctx.empty(V, torch.float64) if want_last else None
    st = _l.BcStats()
    _l.check(ctx.L.vgl_hip_bc_run(ctx.h, graph.h, src, n, int(bool(symmetric)), int(accumulate), _ptr(out), _ptr(levels), _ptr(sigma), _ptr(delta),
                                  C.byref(st)))
    stats = _stats(st)
    to_orig = not (raw or accumulate or graph.fwd is None)
    idx = graph.fwd.long() if to_orig else None                     # 8-byte values: a torch index over the mapping to_original applies
    if want_last:
        stats["levels"] = levels[idx] if to_orig else levels
        stats["sigma"] = sigma[idx] if to_orig else sigma
        stats["delta"] = delta[idx] if to_orig else delta
    if accumulate:
        return out, stats
    if rescale and n:
        out = out * (float(V) / float(n))
    if halve:
        out = out * 0.5
    return (out[idx] if to_orig else out), stats


def _source_ids(graph, sources, raw, who):
    """sources (None = every vertex; ORIGINAL ids unless raw) -> list of ids in the graph's own numbering"""
    V = graph.V
    if sources is None:
        ids = list(range(V))
    else:
        ids = [int(s) for s in (sources.tolist() if torch.is_tensor(sources) else sources)]
    if not raw and graph.fwd is not None and ids:
        if min(ids) < 0 or max(ids) >= V:
            raise _l.VglHipError(who + ": source vertex out of range")
        fwd = graph.fwd.cpu()
        ids = [int(fwd[s]) for s in ids]
    return ids


def multi_source_bfs(graph, sources=None, direction="out", symmetric=False, want_levels=False, raw=False):
    """bit-parallel multi-source BFS (the contract of vgl_hip_msbfs_run in include/vgl_hip.h): 64 traversals per pass over the adjacency.
    sources: None = every vertex, else a sequence / tensor of ORIGINAL vertex ids (raw=True: the graph's own ids); a repeated source is a traversal of
    its own.  direction "out": d(s, v) along stored outgoing entries; "in": along incoming entries (the distance from v to s).  symmetric=True: the
    caller vouches that every edge is stored both ways (no incoming CSR needed).  Returns (dict of per-source tensors in source order -- "reached"
    int64, "dist_sum" int64, "ecc" int32, "harmonic" float64 and, with want_levels, "levels" int32 [len(sources), V] with the columns in ORIGINAL
    order unless raw -- , stats dict)."""
    ctx = graph.ctx
    V = graph.V
    ids = _source_ids(graph, sources, raw, "multi_source_bfs")
    n = len(ids)
    src = (C.c_int32 * max(n, 1))(*ids)
    res = {"reached": ctx.empty(n, torch.int64), "dist_sum": ctx.empty(n, torch.int64), "ecc": ctx.empty(n, torch.int32),
           "harmonic": ctx.empty(n, torch.float64)}
    levels = torch.empty((n, V), dtype=torch.int32, device=ctx.device) if want_levels else None
    st = _l.MsbfsStats()
    _l.check(ctx.L.vgl_hip_msbfs_run(ctx.h, graph.h, src, n, {"out": 0, "in": 1}[direction], int(bool(symmetric)), _ptr(res["reached"]),
                                     _ptr(res["dist_sum"]), _ptr(res["ecc"]), _ptr(res["harmonic"]), _ptr(levels), C.byref(st)))
    if want_levels:
        res["levels"] = levels if (raw or graph.fwd is None) else levels[:, graph.fwd.long()]
    return res, _stats(st)


def closeness_centrality(graph, sources=None, direction="in", symmetric=False, wf_improved=True, raw=False):
    """closeness centrality of `sources` (None = every vertex), float64 in source order: (r - 1) / dist_sum, r = vertices reached, times
    (r - 1) / (V - 1) when wf_improved (Wasserman and Faust), 0 where dist_sum == 0.  The default direction "in" is networkx's convention on a
    directed graph (distances TO the vertex).  Returns (closeness, stats dict)."""
    res, stats = multi_source_bfs(graph, sources, direction, symmetric, raw=raw)
    r1 = (res["reached"] - 1).to(torch.float64)
    tot = res["dist_sum"].to(torch.float64)
    c = torch.where(tot > 0, r1 / torch.clamp(tot, min=1.0), torch.zeros_like(tot))
    if wf_improved and graph.V > 1:
        c = c * (r1 / float(graph.V - 1))
    return c, stats


def harmonic_centrality(graph, sources=None, direction="in", symmetric=False, raw=False):
    """harmonic centrality of `sources` (None = every vertex), float64 in source order: the sum over the other vertices of 1 / d, added level by
    level in ascending d (bit-identical from run to run).  Returns (harmonic, stats dict)."""
    res, stats = multi_source_bfs(graph, sources, direction, symmetric, raw=raw)
    return res["harmonic"], stats


def eccentricity(graph, sources=None, direction="out", symmetric=False, raw=False):
    """the largest finite distance from every source (None = every vertex), int32 in source order.  Returns (eccentricity, stats dict)."""
    res, stats = multi_source_bfs(graph, sources, direction, symmetric, raw=raw)
    return res["ecc"], stats


def personalized_pagerank(graph, seeds, weights=None, alpha=0.85, max_iterations=100, tol=0.0, symmetric=False, raw=False, with_stats=False):
    """batched personalised PageRank (the contract of vgl_hip_ppr_run in include/vgl_hip.h): float64 power iteration with restart at a seed set, up to
    16 seed sets per pass over the incoming entries, dangling mass returned along the teleport vector (networkx's pagerank with
    dangling = personalization).  seeds: a list of lists of ORIGINAL vertex ids (raw=True: the graph's own ids), one list per problem; one flat list
    of ints means one problem per vertex; an EMPTY list is the uniform teleport, i.e. plain PageRank.  weights: None (1 each) or positive numbers in
    the shape of seeds; a vertex listed twice gets both.  tol == 0 runs exactly max_iterations iterations; tol > 0 stops a batch of 16 once its
    largest L1 change is <= tol.  symmetric=True: the caller vouches that every edge is stored both ways (no incoming CSR needed).  page_rank() is
    the reference's float32 benchmark kernel and another function.  Returns rank, float64 [len(seeds), V] with the columns in ORIGINAL order unless
    raw; with_stats: (rank, dict of the stats plus "err" float64 and "iterations" int32 per problem)."""
    ctx = graph.ctx
    V = graph.V
    seeds = seeds.tolist() if torch.is_tensor(seeds) else list(seeds)
    flat = all(not isinstance(s, (list, tuple)) and not torch.is_tensor(s) for s in seeds)
    lists = [[int(s)] for s in seeds] if flat else [[int(v) for v in (s.tolist() if torch.is_tensor(s) else s)] for s in seeds]
    wl = None
    if weights is not None:
        weights = weights.tolist() if torch.is_tensor(weights) else list(weights)
        wl = [[float(w)] for w in weights] if flat else [[float(x) for x in (w.tolist() if torch.is_tensor(w) else w)] for w in weights]
        if [len(w) for w in wl] != [len(s) for s in lists]:
            raise _l.VglHipError("personalized_pagerank: weights must have the shape of seeds")
    ids = [v for s in lists for v in s]
    if not raw and graph.fwd is not None and ids:
        if min(ids) < 0 or max(ids) >= V:
            raise _l.VglHipError("personalized_pagerank: seed vertex out of range")
        fwd = graph.fwd.cpu()
        ids = [int(fwd[v]) for v in ids]
    n = len(lists)
    ptr = [0]
    for s in lists:
        ptr.append(ptr[-1] + len(s))
    c_ids = (C.c_int32 * max(len(ids), 1))(*ids)
    c_ptr = (C.c_int64 * (n + 1))(*ptr)
    c_w = None if wl is None else (C.c_double * max(len(ids), 1))(*[x for w in wl for x in w])
    rank = torch.empty((n, V), dtype=torch.float64, device=ctx.device)
    err = ctx.empty(n, torch.float64)
    its = ctx.empty(n, torch.int32)
    st = _l.PprStats()
    _l.check(ctx.L.vgl_hip_ppr_run(ctx.h, graph.h, c_ids, c_ptr, c_w, n, float(alpha), int(max_iterations), float(tol), int(bool(symmetric)),
                                   _ptr(rank), _ptr(err), _ptr(its), C.byref(st)))
    if not raw and graph.fwd is not None:
        rank = rank[:, graph.fwd.long()]
    if not with_stats:
        return rank
    info = _stats(st)
    info["err"], info["iterations"] = err, its
    return rank, info


def pagerank(graph, alpha=0.85, max_iterations=100, tol=1e-10, symmetric=False, raw=False):
    """plain PageRank as networkx defines it (uniform teleport, dangling mass spread uniformly): the empty-list problem of personalized_pagerank().
    Returns one float64 vector of V values in ORIGINAL order unless raw.  Not page_rank(), the reference's float32 benchmark kernel."""
    return personalized_pagerank(graph, [[]], alpha=alpha, max_iterations=max_iterations, tol=tol, symmetric=symmetric, raw=raw)[0]


def core_numbers(graph, k_limit=0, degree=False, raw=False):
    """k-core decomposition of the simple undirected graph underlying the stored outgoing CSR (the contract of vgl_hip_kcore_run in
    include/vgl_hip.h).  Returns (degeneracy, stats dict); stats["core"] is an int32 tensor: the core number of every vertex, or
    min(core, k_limit) when k_limit > 0 (the peel stops there).  degree=True adds stats["degree"] (int32, undirected simple degree).  Both in
    ORIGINAL vertex order unless raw=True."""
    ctx = graph.ctx
    core = ctx.empty(graph.V, torch.int32)
    deg = ctx.empty(graph.V, torch.int32) if degree else None
    st = _l.KcoreStats()
    _l.check(ctx.L.vgl_hip_kcore_run(ctx.h, graph.h, int(k_limit), _ptr(core), _ptr(deg), C.byref(st)))
    stats = _stats(st)
    stats["core"] = core if raw else graph.to_original(core)
    if degree:
        stats["degree"] = deg if raw else graph.to_original(deg)
    return int(st.degeneracy), stats


def k_core(graph, k, raw=False):
    """membership of the k-core: a bool tensor, True where core >= k; the peel stops at k (core_numbers with k_limit=k).  k >= 1."""
    if int(k) < 1:
        raise _l.VglHipError("k_core: k must be at least 1 (every vertex is in the 0-core)")
    _, stats = core_numbers(graph, k_limit=int(k), raw=raw)
    return stats["core"] >= int(k)


def truss_numbers(graph, k_limit=0, support=False, raw=False):
    """k-truss decomposition of the simple undirected graph underlying the stored outgoing CSR (the contract of vgl_hip_ktruss_run in
    include/vgl_hip.h).  Returns (max_truss, stats dict); stats["edges"] is an int32 tensor [E', 2], the endpoints lo < hi of every undirected edge,
    stats["truss"] an int32 tensor [E']: the truss number of that edge, or min(truss, k_limit) when k_limit >= 2 (the peel stops there).
    support=True adds stats["support"] (int32 [E']: the triangles that contain the edge).  The endpoints are ORIGINAL vertex ids and the rows ascend by
    (lo, hi) unless raw=True, which keeps the graph's own numbering and its edge order."""
    ctx = graph.ctx
    cap = max(graph.E, 1)                                           # E' <= the stored entries: the run itself tells E' (and whether it prepared)
    eu, ev, truss = ctx.empty(cap, torch.int32), ctx.empty(cap, torch.int32), ctx.empty(cap, torch.int32)
    sup = ctx.empty(cap, torch.int32) if support else None
    st = _l.KtrussStats()
    _l.check(ctx.L.vgl_hip_ktruss_run(ctx.h, graph.h, int(k_limit), _ptr(eu), _ptr(ev), _ptr(truss), _ptr(sup), C.byref(st)))
    stats = _stats(st)
    n = int(st.undirected_edges)
    eu, ev, truss = eu[:n], ev[:n], truss[:n]
    sup = sup[:n] if support else None
    if not raw and graph.bwd is not None and n:
        a, b = graph.bwd[eu.long()], graph.bwd[ev.long()]
        eu, ev = torch.minimum(a, b), torch.maximum(a, b)
        order = torch.argsort(eu.long() * graph.V + ev.long())
        eu, ev, truss = eu[order], ev[order], truss[order]
        sup = sup[order] if support else None
    stats["edges"] = torch.stack([eu, ev], dim=1)
    stats["truss"] = truss
    if support:
        stats["support"] = sup
    return int(st.max_truss), stats


def k_truss(graph, k, raw=False):
    """the edges of the k-truss: an int32 tensor [n, 2] of the edges with truss >= k, in the order of truss_numbers(); the peel stops at k
    (truss_numbers with k_limit=k).  k >= 2."""
    if int(k) < 2:
        raise _l.VglHipError("k_truss: k must be at least 2 (every edge is in the 2-truss)")
    _, stats = truss_numbers(graph, k_limit=int(k), raw=raw)
    return stats["edges"][stats["truss"] >= int(k)]


def minimum_spanning_forest(graph, weights, component=False, raw=False):
    """minimum spanning forest of the simple undirected graph underlying the stored outgoing CSR (the contract of vgl_hip_msf_run in
    include/vgl_hip.h); weights: float32, one per stored outgoing entry in CSR order, as sssp() takes them.  Returns (total_weight, stats dict);
    stats["edges"] is an int32 tensor [n, 2], the forest edges lo < hi, stats["weights"] a float32 tensor [n], their weights.  Of ALL E' undirected
    edges, in the same numbering and order: stats["all_edges"] (int32 [E', 2]), stats["edge_weight"] (float32 [E'], the lightest stored copy) and
    stats["in_forest"] (bool [E']).  component=True adds stats["component"] (int32 [V]): one representative vertex per component (the smallest id
    in the graph's own numbering).  all_edges / edge_weight / in_forest go beyond the forest itself: the run fills them anyway (the library writes
    the mask and, on request, endpoints and folded weights per undirected edge; the four result arrays are sized by the stored entries, 13 bytes
    each, because E' is known only after the run), and the tests compare them.  Endpoints and representatives are ORIGINAL vertex ids, the edges ascend by (lo, hi) and component is in
    ORIGINAL vertex order unless raw=True, which keeps the graph's own numbering and its edge order."""
    ctx = graph.ctx
    cap = max(graph.E, 1)                                           # E' <= the stored entries: the run itself tells E' (and whether it prepared)
    eu, ev = ctx.empty(cap, torch.int32), ctx.empty(cap, torch.int32)
    ew, mask = ctx.empty(cap, torch.float32), ctx.empty(cap, torch.uint8)
    comp = ctx.empty(graph.V, torch.int32) if component else None
    st = _l.MsfStats()
    _l.check(ctx.L.vgl_hip_msf_run(ctx.h, graph.h, _ptr(weights), _ptr(eu), _ptr(ev), _ptr(ew), _ptr(mask), _ptr(comp), C.byref(st)))
    stats = _stats(st)
    n = int(st.undirected_edges)
    eu, ev, ew, mask = eu[:n], ev[:n], ew[:n], mask[:n].bool()
    to_orig = not raw and graph.bwd is not None
    if to_orig and n:
        a, b = graph.bwd[eu.long()], graph.bwd[ev.long()]
        eu, ev = torch.minimum(a, b), torch.maximum(a, b)
        order = torch.argsort(eu.long() * graph.V + ev.long())
        eu, ev, ew, mask = eu[order], ev[order], ew[order], mask[order]
    stats["all_edges"] = torch.stack([eu, ev], dim=1)
    stats["edge_weight"] = ew
    stats["in_forest"] = mask
    stats["edges"] = stats["all_edges"][mask]
    stats["weights"] = ew[mask]
    if component:
        stats["component"] = graph.to_original(graph.bwd[comp.long()]) if to_orig else comp
    return float(st.total_weight), stats


def _bicc(graph, raw, edges=False, bridge=False, edge_component=False, articulation=False, two_edge_component=False):
    """one vgl_hip_bicc_run with the outputs named; what is not named goes as NULL.  Returns the stats dict with the tensors asked for."""
    ctx = graph.ctx
    cap = max(graph.E, 1)                                           # E' <= the stored entries: the run itself tells E' (and whether it prepared)
    eu = ctx.empty(cap, torch.int32) if edges else None
    ev = ctx.empty(cap, torch.int32) if edges else None
    br = ctx.empty(cap, torch.uint8) if bridge else None
    lab = ctx.empty(cap, torch.int32) if edge_component else None
    art = ctx.empty(graph.V, torch.uint8) if articulation else None
    two = ctx.empty(graph.V, torch.int32) if two_edge_component else None
    st = _l.BiccStats()
    _l.check(ctx.L.vgl_hip_bicc_run(ctx.h, graph.h, _ptr(eu), _ptr(ev), _ptr(br), _ptr(lab), _ptr(art), _ptr(two), C.byref(st)))
    stats = _stats(st)
    n = int(st.undirected_edges)
    to_orig = not raw and graph.bwd is not None
    order = None
    if edges:
        eu, ev = eu[:n], ev[:n]
        if to_orig and n:
            a, b = graph.bwd[eu.long()], graph.bwd[ev.long()]
            eu, ev = torch.minimum(a, b), torch.maximum(a, b)
            order = torch.argsort(eu.long() * graph.V + ev.long())
            eu, ev = eu[order], ev[order]
        stats["edges"] = torch.stack([eu, ev], dim=1)
    if bridge:
        br = br[:n].bool()
        stats["bridge"] = br[order] if order is not None else br
    if edge_component:
        lab = lab[:n]
        if order is not None:                                         # canonical again: the smallest row, in the returned order, of the block
            lab = lab[order].long()
            first = torch.full((n,), n, dtype=torch.int64, device=ctx.device)
            first.scatter_reduce_(0, lab, torch.arange(n, device=ctx.device), "amin")
            lab = first[lab].to(torch.int32)
        stats["edge_component"] = lab
    if articulation:
        art = art.bool()
        stats["articulation"] = graph.to_original(art.to(torch.int32)).bool() if to_orig else art
    if two_edge_component:
        if to_orig:                                                   # canonical again: the smallest ORIGINAL id of the component
            lab = two.long()
            first = torch.full((graph.V,), graph.V, dtype=torch.int64, device=ctx.device)
            first.scatter_reduce_(0, lab, graph.bwd.long(), "amin")
            two = graph.to_original(first[lab].to(torch.int32))
        stats["two_edge_component"] = two
    return stats


def biconnected_components(graph, raw=False):
    """bridges, cut vertices, biconnected components (blocks) and 2-edge-connected components of the simple undirected graph underlying the stored
    outgoing CSR (the contract of vgl_hip_bicc_run in include/vgl_hip.h).  Returns (number of blocks, stats dict); of the E' undirected edges:
    stats["edges"] (int32 [E', 2], lo < hi), stats["edge_component"] (int32 [E']: the block of the edge, named by the smallest row index of an
    edge of that block), stats["bridge"] (bool [E']); of the vertices: stats["articulation"] (bool [V]) and stats["two_edge_component"] (int32 [V]:
    the smallest vertex id of the vertex's component once the bridges are removed).  Endpoints and vertex arrays are in ORIGINAL ids, the edges ascend
    by (lo, hi) and both labellings are canonical in that numbering unless raw=True, which keeps the graph's own numbering and its edge order."""
    stats = _bicc(graph, raw, edges=True, bridge=True, edge_component=True, articulation=True, two_edge_component=True)
    return int(stats["biconnected_components"]), stats


def bridges(graph, raw=False):
    """the bridges of that graph: an int32 tensor [n, 2], lo < hi, in the order of biconnected_components(); the block pass is skipped"""
    stats = _bicc(graph, raw, edges=True, bridge=True)
    return stats["edges"][stats["bridge"]]


def articulation_points(graph, raw=False):
    """the cut vertices of that graph: ascending vertex ids (int64), ORIGINAL unless raw=True"""
    stats = _bicc(graph, raw, articulation=True)
    return torch.nonzero(stats["articulation"]).flatten()


def two_edge_connected_components(graph, raw=False):
    """int32 [V]: the smallest vertex id of every vertex's 2-edge-connected component (ORIGINAL ids and vertex order unless raw=True); the block pass
    is skipped"""
    return _bicc(graph, raw, two_edge_component=True)["two_edge_component"]


def _fmix32(h):
    """the murmur3 finaliser on an int64 tensor of uint32 values"""
    m = 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x85ebca6b) & m
    h = h ^ (h >> 13)
    h = (h * 0xc2b2ae35) & m
    return h ^ (h >> 16)


def priority_key(ids, seed=0):
    """key(i, seed) = fmix32(i ^ fmix32(seed + 0x9e3779b9)) of include/vgl_hip.h for an integer tensor of ids: int64 values in [0, 2^32)"""
    mix = _fmix32(torch.tensor([(int(seed) + 0x9e3779b9) & 0xFFFFFFFF], dtype=torch.int64, device=ids.device))
    return _fmix32((ids.to(torch.int64) & 0xFFFFFFFF) ^ mix)


def _as_u32(ctx, values, n, who):
    """n uint32 priorities as the int32 tensor of their bit patterns, on the context's device"""
    p = torch.as_tensor(values).to(ctx.device).to(torch.int64).flatten()
    if p.numel() != n:
        raise _l.VglHipError("%s: %d priorities for %d items" % (who, p.numel(), n))
    if n and (int(p.min()) < 0 or int(p.max()) > 0xFFFFFFFF):
        raise _l.VglHipError("%s: priorities are uint32 values" % who)
    return torch.where(p >= (1 << 31), p - (1 << 32), p).to(torch.int32).contiguous()


def maximal_independent_set(graph, priority=None, seed=0, rounds=False, raw=False):
    """the lexicographically first maximal independent set of the simple undirected graph underlying the stored outgoing CSR, under the order
    (priority, id) ascending (the contract of vgl_hip_mis_run in include/vgl_hip.h): what the sequential greedy algorithm returns.  Returns
    (size, stats dict); stats["in_set"] is a bool tensor [V]; rounds=True adds stats["round"] (int32 [V]: +r entered in round r, -r excluded in round
    r).  priority: V uint32 values (any integer tensor or array), smaller first, ties to the smaller id in the graph's own numbering; None: the
    library's key(id, seed).  priority and both outputs are in ORIGINAL vertex order, and the default keys are those of the ORIGINAL ids (built here
    and passed for a renumbered graph), so the default result does not depend on renumber=; raw=True keeps the graph's own numbering throughout."""
    ctx = graph.ctx
    to_orig = not raw and graph.bwd is not None
    prio = None
    if priority is not None:
        prio = _as_u32(ctx, priority, graph.V, "maximal_independent_set")
        if to_orig:
            prio = prio[graph.bwd.long()].contiguous()
    elif to_orig:
        prio = _as_u32(ctx, priority_key(graph.bwd, seed), graph.V, "maximal_independent_set")
    in_set = ctx.empty(max(graph.V, 1), torch.uint8)[:graph.V]      # (never a NULL pointer: an empty graph is no refusal)
    rnd = ctx.empty(max(graph.V, 1), torch.int32)[:graph.V] if rounds else None
    st = _l.MisStats()
    _l.check(ctx.L.vgl_hip_mis_run(ctx.h, graph.h, _ptr(prio), int(seed) & 0xFFFFFFFF, _ptr(in_set), _ptr(rnd), C.byref(st)))
    stats = _stats(st)
    stats["in_set"] = graph.to_original(in_set.to(torch.int32)).bool() if to_orig else in_set.bool()
    if rounds:
        stats["round"] = graph.to_original(rnd) if to_orig else rnd
    return int(st.set_size), stats


def maximal_matching(graph, edge_priority=None, seed=0, raw=False):
    """the lexicographically first maximal matching of that graph under the order (priority, edge id) ascending over the library's edge numbering
    (the contract of vgl_hip_matching_run in include/vgl_hip.h): what the sequential greedy algorithm over the edges returns.  Returns
    (matched edges, stats dict); stats["edges"] is an int32 tensor [E', 2], lo < hi, stats["in_matching"] a bool tensor [E'], stats["mate"] an int32
    tensor [V] (the partner, or -1) and stats["round"] an int32 tensor [V] (the round in which the vertex was matched, or 0).  Endpoints and mates are
    ORIGINAL vertex ids, the edges ascend by (lo, hi) and the vertex arrays are in ORIGINAL order unless raw=True.  edge_priority (E' uint32 values)
    and the default keys key(edge id, seed) follow THE GRAPH'S OWN edge numbering -- the row order of stats["edges"] under raw=True -- so on a renumbered
    graph the default matching differs from that of the same graph without renumber=; it is the greedy matching either way."""
    ctx = graph.ctx
    cap = max(graph.E, 1)                                           # E' <= the stored entries: the run itself tells E' (and whether it prepared)
    prio = None
    if edge_priority is not None:
        prio = _as_u32(ctx, edge_priority, graph.prepare_matching(), "maximal_matching")
    eu, ev, mask = ctx.empty(cap, torch.int32), ctx.empty(cap, torch.int32), ctx.empty(cap, torch.uint8)
    mate, rnd = ctx.empty(max(graph.V, 1), torch.int32)[:graph.V], ctx.empty(max(graph.V, 1), torch.int32)[:graph.V]
    st = _l.MatchingStats()
    _l.check(ctx.L.vgl_hip_matching_run(ctx.h, graph.h, _ptr(prio), int(seed) & 0xFFFFFFFF, _ptr(eu), _ptr(ev), _ptr(mask), _ptr(mate), _ptr(rnd), C.byref(st)))
    stats = _stats(st)
    n = int(st.undirected_edges)
    eu, ev, mask = eu[:n], ev[:n], mask[:n].bool()
    if not raw and graph.bwd is not None:
        if n:
            a, b = graph.bwd[eu.long()], graph.bwd[ev.long()]
            eu, ev = torch.minimum(a, b), torch.maximum(a, b)
            order = torch.argsort(eu.long() * graph.V + ev.long())
            eu, ev, mask = eu[order], ev[order], mask[order]
        partner = torch.where(mate >= 0, graph.bwd[mate.clamp(min=0).long()], mate)
        mate, rnd = graph.to_original(partner.contiguous()), graph.to_original(rnd)
    stats["edges"] = torch.stack([eu, ev], dim=1)
    stats["in_matching"] = mask
    stats["mate"] = mate
    stats["round"] = rnd
    return int(st.matched_edges), stats


def vertex_cover(graph, edge_priority=None, seed=0, raw=False):
    """a vertex cover of that graph of at most twice the minimum size: the matched vertices (mate >= 0) of maximal_matching(); a bool tensor [V]"""
    return maximal_matching(graph, edge_priority=edge_priority, seed=seed, raw=raw)[1]["mate"] >= 0


SIM_COMMON, SIM_JACCARD, SIM_OVERLAP, SIM_MAX_K = 0, 1, 2, 64
_SIM_CODES = {"common": SIM_COMMON, "jaccard": SIM_JACCARD, "overlap": SIM_OVERLAP, "sorensen": SIM_JACCARD}      # Sorensen ranks exactly as Jaccard


def _pair_ids(graph, pairs, raw, who):
    """pairs ([n, 2]: tensor, array or sequence; ORIGINAL ids unless raw) -> (u, v), int32 device tensors in the graph's own numbering"""
    p = torch.as_tensor(pairs).to(graph.ctx.device).to(torch.int64).reshape(-1, 2)
    if p.numel():
        lo, hi = int(p.min()), int(p.max())
        if lo < -(1 << 31) or hi >= (1 << 31) or (not raw and graph.fwd is not None and (lo < 0 or hi >= graph.V)):
            raise _l.VglHipError(who + ": a vertex of a pair is out of range")
        if not raw and graph.fwd is not None:
            p = graph.fwd[p]
    return p[:, 0].to(torch.int32).contiguous(), p[:, 1].to(torch.int32).contiguous()


def _sim_pairs(graph, u, v, weight=None, common=True, degree=False):
    """one vgl_hip_sim_pairs over pairs in the graph's own numbering; returns (common or None, weighted or None, degree or None, stats dict)"""
    ctx = graph.ctx
    n = int(u.numel())
    c = ctx.empty(max(n, 1), torch.int32) if common else None        # (never a NULL pointer: no pairs is no refusal)
    w = ctx.empty(max(n, 1), torch.float64) if weight is not None else None
    deg = ctx.empty(graph.V, torch.int32) if degree else None
    st = _l.SimPairsStats()
    _l.check(ctx.L.vgl_hip_sim_pairs(ctx.h, graph.h, _ptr(u), _ptr(v), n, _ptr(weight), _ptr(c), _ptr(w), _ptr(deg), C.byref(st)))
    return c[:n] if common else None, w[:n] if weight is not None else None, deg, _stats(st)


def _sim_degree(graph):
    """d(v) in the graph's own numbering: a vgl_hip_sim_pairs call without pairs writes nothing else"""
    none = graph.ctx.empty(0, torch.int32)
    return _sim_pairs(graph, none, none, degree=True)[2]


def _sim_score(metric, c, du, dv):
    """the float64 score of `metric` from the common neighbours and the two degrees; 0 where the denominator is 0"""
    c, du, dv = c.to(torch.float64), du.to(torch.float64), dv.to(torch.float64)
    if metric == "common":
        return c
    if metric == "jaccard":
        num, den = c, du + dv - c
    elif metric == "overlap":
        num, den = c, torch.minimum(du, dv)
    elif metric == "sorensen":
        num, den = 2.0 * c, du + dv
    else:
        raise _l.VglHipError("similarity: unknown metric %r" % (metric,))
    return torch.where(den > 0, num / torch.clamp(den, min=1.0), torch.zeros_like(den))


def common_neighbors(graph, pairs, raw=False):
    """c(u, v) = |N(u) & N(v)| in the simple undirected graph underlying the stored outgoing CSR (the contract of vgl_hip_sim_pairs in
    include/vgl_hip.h) for every row of pairs ([n, 2], ORIGINAL vertex ids unless raw=True; any order, repeats and u == v allowed): int32 [n]"""
    u, v = _pair_ids(graph, pairs, raw, "common_neighbors")
    return _sim_pairs(graph, u, v)[0]


def similarity(graph, pairs, metric="jaccard", raw=False):
    """the similarity of every pair: "jaccard" c / (d(u) + d(v) - c), "overlap" c / min(d(u), d(v)), "sorensen" 2 c / (d(u) + d(v)), float64 [n], built
    with torch from the library's common-neighbour counts and degrees, 0 where the denominator is 0.  Returns (scores, stats dict); stats["common"]
    is the int32 [n] count per pair, stats["degree"] the int32 [V] degrees (ORIGINAL vertex order unless raw=True)."""
    if metric not in ("jaccard", "overlap", "sorensen"):
        raise _l.VglHipError("similarity: unknown metric %r" % (metric,))
    u, v = _pair_ids(graph, pairs, raw, "similarity")
    c, _, deg, stats = _sim_pairs(graph, u, v, degree=True)
    stats["common"] = c
    stats["degree"] = deg if raw else graph.to_original(deg)
    return _sim_score(metric, c, deg[u.long()], deg[v.long()]), stats


def _weighted_common(graph, pairs, raw, who, weight_of_degree):
    u, v = _pair_ids(graph, pairs, raw, who)
    deg = _sim_degree(graph)
    c, w, _, stats = _sim_pairs(graph, u, v, weight=weight_of_degree(deg.to(torch.float64)).contiguous())
    stats["common"] = c
    stats["degree"] = deg if raw else graph.to_original(deg)
    return w, stats


def adamic_adar(graph, pairs, raw=False):
    """the Adamic-Adar index of every pair: the sum over the common neighbours w of 1 / ln d(w) (a vertex with d(w) < 2 weighs 0; a common neighbour
    has d >= 2 unless u == v), float64 [n].  The weights are built here in float64 from the library's degrees; the sum is the library's
    (vgl_hip_sim_pairs, d_weighted: one writer per pair, a fixed summation shape).  Returns (scores, stats dict) as similarity() does."""
    return _weighted_common(graph, pairs, raw, "adamic_adar",
                            lambda d: torch.where(d >= 2, 1.0 / torch.log(torch.clamp(d, min=2.0)), torch.zeros_like(d)))


def resource_allocation(graph, pairs, raw=False):
    """the resource-allocation index of every pair: the sum over the common neighbours w of 1 / d(w) (0 where d(w) < 1), float64 [n]; see adamic_adar()"""
    return _weighted_common(graph, pairs, raw, "resource_allocation",
                            lambda d: torch.where(d >= 1, 1.0 / torch.clamp(d, min=1.0), torch.zeros_like(d)))


def edge_similarity(graph, metric="jaccard", raw=False):
    """the similarity of the two ends of all E' undirected edges, in the library's edge numbering (taken from truss_numbers(), whose peel stops at
    once).  metric: "common", "jaccard", "overlap" or "sorensen".  Returns (scores float64 [E'], stats dict); stats["edges"] is the int32 [E', 2]
    tensor of the endpoints lo < hi and stats["common"] the int32 [E'] counts (the triangle support of the edge), ordered like truss_numbers():
    ORIGINAL ids ascending by (lo, hi) unless raw=True."""
    edges = truss_numbers(graph, k_limit=2, raw=True)[1]["edges"]
    eu, ev = edges[:, 0].contiguous(), edges[:, 1].contiguous()
    c, _, deg, stats = _sim_pairs(graph, eu, ev, degree=True)
    score = _sim_score(metric, c, deg[eu.long()], deg[ev.long()])
    if not raw and graph.bwd is not None and eu.numel():
        a, b = graph.bwd[eu.long()], graph.bwd[ev.long()]
        eu, ev = torch.minimum(a, b), torch.maximum(a, b)
        order = torch.argsort(eu.long() * graph.V + ev.long())
        eu, ev, c, score = eu[order], ev[order], c[order], score[order]
    stats["edges"] = torch.stack([eu, ev], dim=1)
    stats["common"] = c
    return score, stats


def link_prediction(graph, k=10, metric="jaccard", vertices=None, include_neighbors=False, raw=False):
    """for every query vertex the k most similar vertices of its 2-hop neighbourhood (the contract of vgl_hip_sim_topk in include/vgl_hip.h): the
    candidates are the w != u with a common neighbour, without N(u) unless include_neighbors; metric "common", "jaccard", "overlap" or "sorensen"
    (which ranks as Jaccard); the scores are compared as exact fractions and equal scores go to the smaller ORIGINAL id (raw=True: the smaller id of
    the graph's own numbering), so the answer does not depend on renumber=.  vertices: None = every vertex in id order, else ORIGINAL ids (raw=True:
    the graph's own), repeats allowed.  Returns (ids int32 [n, k] best first, padded with -1; common int32 [n, k], padded with 0; score float64
    [n, k], 0 in the padding; stats dict)."""
    ctx = graph.ctx
    if metric not in _SIM_CODES:
        raise _l.VglHipError("link_prediction: unknown metric %r" % (metric,))
    to_orig = not raw and graph.bwd is not None
    if vertices is None:
        q = graph.fwd.contiguous() if to_orig else None              # row i is ORIGINAL vertex i
        n = graph.V
    else:
        ids = _source_ids(graph, vertices, raw, "link_prediction")
        n = len(ids)
        q = torch.tensor(ids, dtype=torch.int32, device=ctx.device) if n else ctx.empty(1, torch.int32)
    kk = int(k)
    cells = max(n * max(kk, 1), 1)
    ids_out, common = ctx.empty(cells, torch.int32), ctx.empty(cells, torch.int32)
    st = _l.SimTopkStats()
    _l.check(ctx.L.vgl_hip_sim_topk(ctx.h, graph.h, _ptr(q), n, _SIM_CODES[metric], kk, int(bool(include_neighbors)),
                                    _ptr(graph.bwd.contiguous()) if to_orig else None, _ptr(ids_out), _ptr(common), C.byref(st)))
    ids_out, common = ids_out[:n * kk].reshape(n, kk), common[:n * kk].reshape(n, kk)
    deg = _sim_degree(graph)
    own = (graph.fwd if to_orig else torch.arange(graph.V, dtype=torch.int32, device=ctx.device)) if q is None else q[:n]
    held = ids_out >= 0
    du = deg[own.long()][:, None].expand(n, kk)
    dw = deg[ids_out.clamp(min=0).long()]
    score = torch.where(held, _sim_score(metric, common, du, dw), torch.zeros((n, kk), dtype=torch.float64, device=ctx.device))
    if to_orig:
        ids_out = torch.where(held, graph.bwd[ids_out.clamp(min=0).long()], ids_out)
    return ids_out, common, score, _stats(st)


def _seed_ids(graph, seeds, raw, who):
    """seeds (tensor, array or sequence; ORIGINAL ids unless raw; repeats allowed) -> int32 device tensor in the graph's own numbering (never an empty
    allocation) and their number"""
    s = torch.as_tensor(seeds).to(graph.ctx.device).to(torch.int64).flatten()
    n = int(s.numel())
    if n:
        lo, hi = int(s.min()), int(s.max())
        if lo < -(1 << 31) or hi >= (1 << 31) or (not raw and graph.fwd is not None and (lo < 0 or hi >= graph.V)):
            raise _l.VglHipError(who + ": a seed is out of range")
        if not raw and graph.fwd is not None:
            s = graph.fwd[s]
    return (s.to(torch.int32).contiguous() if n else graph.ctx.empty(1, torch.int32)), n


def _vertex_keep(graph, vertices_or_mask, raw, who):
    """a bool tensor of V flags or a list of vertex ids (ORIGINAL unless raw) -> uint8 [V] flags in the graph's own numbering"""
    ctx, V = graph.ctx, graph.V
    t = torch.as_tensor(vertices_or_mask).to(ctx.device)
    to_own = not raw and graph.fwd is not None
    if t.dtype == torch.bool:
        if t.numel() != V:
            raise _l.VglHipError("%s: a mask of %d flags for %d vertices" % (who, t.numel(), V))
        keep = t.flatten().to(torch.uint8)
        return (keep[graph.bwd.long()] if to_own else keep).contiguous()
    ids = t.to(torch.int64).flatten()
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= V):
        raise _l.VglHipError(who + ": a vertex is out of range")
    keep = torch.zeros(V, dtype=torch.uint8, device=ctx.device)
    keep[graph.fwd[ids].long() if to_own else ids] = 1
    return keep


def _row_filter(graph, keep_vertex, keep_entry, with_incoming, origin, raw, who):
    """one plan and its fills (vgl_hip_subgraph_plan_* in include/vgl_hip.h) over masks in the graph's own numbering; returns the new Graph"""
    ctx = graph.ctx
    want_in = (graph.in_rowptr is not None) if with_incoming is None else bool(with_incoming)
    if want_in and graph.in_rowptr is None and keep_entry is None:
        raise _l.VglHipError(who + ": with_incoming needs the incoming CSR of the parent")
    plan = C.c_void_p()
    _l.check(ctx.L.vgl_hip_subgraph_plan_create(ctx.h, graph.h, _ptr(keep_vertex), _ptr(keep_entry), C.byref(plan)))
    try:
        vk, eo, ei, st = C.c_int32(), C.c_int64(), C.c_int64(), _l.SubgraphStats()
        _l.check(ctx.L.vgl_hip_subgraph_plan_info(plan, C.byref(vk), C.byref(eo), C.byref(ei), C.byref(st)))
        vk, eo, ei = vk.value, eo.value, ei.value
        if vk == 0:
            raise _l.VglHipError(who + ": no vertex is kept (a graph handle holds at least one vertex)")
        old = ctx.empty(vk, torch.int32)
        _l.check(ctx.L.vgl_hip_subgraph_plan_vertex_maps(ctx.h, plan, None, _ptr(old)))
        rowptr, adj = ctx.empty(vk + 1, torch.int64), ctx.empty(max(eo, 1), torch.int32)
        org = ctx.empty(max(eo, 1), torch.int64) if origin else None
        _l.check(ctx.L.vgl_hip_subgraph_plan_fill(ctx.h, plan, 0, _ptr(rowptr), _ptr(adj), _ptr(org)))
        adj = adj[:eo]
        in_rowptr = in_adj = None
        if want_in and keep_entry is None:
            in_rowptr, in_adj = ctx.empty(vk + 1, torch.int64), ctx.empty(max(ei, 1), torch.int32)
            _l.check(ctx.L.vgl_hip_subgraph_plan_fill(ctx.h, plan, 1, _ptr(in_rowptr), _ptr(in_adj), None))
            in_adj = in_adj[:ei]
        elif want_in:                                                 # an entry mask: the transposition of Graph.from_coo
            csr_src = torch.repeat_interleave(torch.arange(vk, device=ctx.device, dtype=torch.int32), rowptr[1:] - rowptr[:-1])
            in_rowptr, in_adj, _ = ctx.coo_to_csr(vk, adj, csr_src)
    finally:
        ctx.L.vgl_hip_subgraph_plan_destroy(ctx.h, plan)
    sub = Graph(ctx, vk, rowptr, adj, in_rowptr, in_adj)
    sub.parent_ids = old if raw or graph.bwd is None else graph.bwd[old.long()]
    sub.origin = org[:eo] if origin else None
    sub.stats = _stats(st)
    return sub


def induced_subgraph(graph, vertices_or_mask, with_incoming=None, origin=False, raw=False):
    """the subgraph induced by a vertex set (the contract of vgl_hip_subgraph_plan_create in include/vgl_hip.h): a bool tensor of V flags or a list of
    vertex ids, ORIGINAL unless raw=True.  Returns a Graph that owns its tensors; its vertex i is the i-th kept vertex in the PARENT'S OWN numbering,
    its rows hold the parent's entries between kept vertices in their stored order (self-loops and repeated entries included), bit-identical to
    Graph.from_coo on the filtered edge list.  sub.parent_ids (int32 [V']) holds the parent's ORIGINAL id of every vertex (its own id under raw=True);
    sub.origin (int64 [E'], with origin=True) the position of every outgoing entry in the parent's out_adj (weights follow with ctx.gather_u32);
    sub.stats the plan's stats; sub.fwd / sub.bwd are None.  with_incoming: None = as the parent.  Raises VglHipError when no vertex is kept."""
    return _row_filter(graph, _vertex_keep(graph, vertices_or_mask, raw, "induced_subgraph"), None, with_incoming, origin, raw, "induced_subgraph")


def edge_subgraph(graph, entry_mask, with_incoming=None, origin=False, raw=False):
    """the subgraph of an entry mask: one flag per stored outgoing entry in CSR order (bool or integer, nonzero = keep), as sssp() takes weights.  All V
    vertices stay and keep their ids; see induced_subgraph() for what is returned.  The incoming CSR is rebuilt from the result by the transposition
    of Graph.from_coo (with_incoming: None = as the parent)."""
    ctx = graph.ctx
    keep = torch.as_tensor(entry_mask).to(ctx.device).flatten()
    if keep.numel() != graph.E:
        raise _l.VglHipError("edge_subgraph: a mask of %d flags for %d entries" % (keep.numel(), graph.E))
    keep = (keep != 0).to(torch.uint8).contiguous()
    if graph.E == 0:
        keep = torch.zeros(1, dtype=torch.uint8, device=ctx.device)   # (never a NULL pointer)
    return _row_filter(graph, None, keep, with_incoming, origin, raw, "edge_subgraph")


def _k_hop_raw(graph, s, n, hops, direction, symmetric):
    ctx = graph.ctx
    hop = ctx.empty(graph.V, torch.int32)
    st = _l.KhopStats()
    _l.check(ctx.L.vgl_hip_khop_run(ctx.h, graph.h, _ptr(s), n, int(hops), {"out": 0, "in": 1}[direction], int(bool(symmetric)), _ptr(hop), C.byref(st)))
    return hop, _stats(st)


def k_hop(graph, seeds, hops, direction="out", symmetric=False, raw=False, with_stats=False):
    """bounded multi-seed reach (the contract of vgl_hip_khop_run in include/vgl_hip.h): int32 [V], the smallest number of steps from any seed to the
    vertex if that is <= hops, else -1.  seeds: ORIGINAL ids unless raw=True, repeats allowed, may be empty; direction "out" follows stored outgoing
    entries, "in" incoming ones; symmetric=True follows both (needs the incoming CSR).  The array is in ORIGINAL vertex order unless raw=True.
    with_stats=True returns (hop, stats dict)."""
    s, n = _seed_ids(graph, seeds, raw, "k_hop")
    hop, stats = _k_hop_raw(graph, s, n, hops, direction, symmetric)
    hop = hop if raw else graph.to_original(hop)
    return (hop, stats) if with_stats else hop


def ego_graph(graph, seeds, hops, direction="out", symmetric=False, with_incoming=None, origin=False, raw=False):
    """the k-hop (ego) network of a seed set: k_hop() followed by induced_subgraph() on the vertices it reaches.  Returns the Graph of
    induced_subgraph(); sub.hop (int32 [V']) is the hop count of every kept vertex."""
    s, n = _seed_ids(graph, seeds, raw, "ego_graph")
    hop, _ = _k_hop_raw(graph, s, n, hops, direction, symmetric)
    sub = _row_filter(graph, (hop >= 0).to(torch.uint8), None, with_incoming, origin, raw, "ego_graph")
    own = sub.parent_ids if raw or graph.fwd is None else graph.fwd[sub.parent_ids.long()]
    sub.hop = hop[own.long()]
    return sub


def _sample_raw(graph, s, n, fanout, seed, direction, origin):
    ctx = graph.ctx
    cap = max(n * max(int(fanout), 1), 1)
    rowptr, adj = ctx.empty(n + 1, torch.int64), ctx.empty(cap, torch.int32)
    org = ctx.empty(cap, torch.int64) if origin else None
    st = _l.SampleStats()
    _l.check(ctx.L.vgl_hip_sample_neighbors(ctx.h, graph.h, _ptr(s), n, int(fanout), {"out": 0, "in": 1}[direction], int(seed) & 0xFFFFFFFF, _ptr(rowptr),
                                            _ptr(adj), _ptr(org), C.byref(st)))
    total = int(st.sampled_total)
    return rowptr, adj[:total], (org[:total] if origin else None), _stats(st)


def sample_neighbors(graph, seeds, fanout, seed=0, direction="out", origin=False, raw=False):
    """fixed-fanout neighbour sampling without replacement (the contract of vgl_hip_sample_neighbors in include/vgl_hip.h): row i holds the
    min(fanout, degree) entries of the row of seeds[i] with the smallest priority_key(position, seed), in ascending position.  seeds: ORIGINAL ids
    unless raw=True, repeats allowed (each a row of its own).  Returns (rowptr int64 [n + 1], adj int32 [rowptr[n]][, origin int64], stats dict); adj is
    in ORIGINAL ids unless raw=True, origin (with origin=True) the positions in the graph's out_adj / in_adj.  The sample is unique for a given graph
    object but follows ITS numbering: a renumbered graph draws another sample."""
    s, n = _seed_ids(graph, seeds, raw, "sample_neighbors")
    rowptr, adj, org, stats = _sample_raw(graph, s, n, fanout, seed, direction, origin)
    if not raw and graph.bwd is not None:
        adj = graph.bwd[adj.long()]
    return (rowptr, adj, org, stats) if origin else (rowptr, adj, stats)


def sample_blocks(graph, seeds, fanouts, seed=0, direction="out", raw=False):
    """layered sampling for mini-batches: hop h samples fanouts[h] neighbours with the seed `seed + h` for every vertex of its frontier; frontier 0 is
    `seeds` as given, frontier h + 1 the sorted unique union (in the graph's own numbering) of frontier h and its samples.  Returns one dict per hop:
    "seeds" (int32, the frontier), "rowptr" (int64), "adj" (int32) and "stats"; ids are ORIGINAL unless raw=True."""
    front, n = _seed_ids(graph, seeds, raw, "sample_blocks")
    front = front[:n]
    to_orig = not raw and graph.bwd is not None
    blocks = []
    for h, fanout in enumerate(fanouts):
        n = int(front.numel())
        rowptr, adj, _, stats = _sample_raw(graph, front if n else graph.ctx.empty(1, torch.int32), n, fanout, int(seed) + h, direction, False)
        blocks.append({"seeds": graph.bwd[front.long()] if to_orig else front, "rowptr": rowptr, "adj": graph.bwd[adj.long()] if to_orig else adj,
                       "stats": stats})
        front = torch.unique(torch.cat([front, adj])).to(torch.int32).contiguous()
    return blocks


def _own_labels(graph, labels, raw, who):
    """labels (integer tensor or sequence of V entries, in ORIGINAL vertex order unless raw) -> int32 [V] in the graph's own order"""
    lab = torch.as_tensor(labels).to(graph.ctx.device).flatten()
    if lab.is_floating_point() or lab.dtype == torch.bool:
        raise _l.VglHipError(who + ": labels must be integers")
    if lab.numel() != graph.V:
        raise _l.VglHipError("%s: %d labels for %d vertices" % (who, lab.numel(), graph.V))
    lab = lab.to(torch.int64)
    if int(lab.min()) < 0 or int(lab.max()) >= (1 << 31):
        raise _l.VglHipError(who + ": a label is negative or does not fit int32")
    lab = lab.to(torch.int32).contiguous()
    return lab if raw or graph.bwd is None else graph.ctx.permute(graph.bwd, lab)


def quotient_graph(graph, labels, weights=None, self_loops=True, with_incoming=None, raw=False):
    """the quotient graph of a labelling (the contract of vgl_hip_quotient_plan_create in include/vgl_hip.h): the vertices with one label merge into
    one coarse vertex, the stored entries between two labels into one coarse entry.  labels: an integer tensor of V entries >= 0 in ORIGINAL vertex
    order unless raw=True -- the order in which connected_components, strongly_connected_components and label_propagation hand theirs back; coarse
    vertex c stands for the c-th smallest label value.  weights: int64 per stored outgoing entry in CSR order (as sssp takes weights); None = 1
    each.  self_loops=False leaves out the entries inside a cluster.  Returns a Graph that owns its tensors, every row ascending and free of repeats,
    bit-identical to Graph.from_coo on the ascending list of distinct coarse pairs; q.count (int64 [E']) the summed weight (the multiplicity) of every
    outgoing entry, q.in_count of every incoming one when the incoming CSR is built (with_incoming: None = as the parent); q.label_of (int32 [V']),
    q.size (int32 [V']), q.cluster_of (int32 [V], in ORIGINAL order unless raw=True), q.stats; q.fwd / q.bwd are None.  Without weights the incoming
    CSR is filled by the same kernels over the parent's incoming CSR; with weights, or when the parent has none, it is the transposition
    Graph.from_coo uses and in_count follows its permutation."""
    ctx = graph.ctx
    lab = _own_labels(graph, labels, raw, "quotient_graph")
    want_in = (graph.in_rowptr is not None) if with_incoming is None else bool(with_incoming)
    w = None
    if weights is not None:
        w = torch.as_tensor(weights).to(ctx.device).flatten()
        if w.is_floating_point():
            raise _l.VglHipError("quotient_graph: weights must be integers")
        if w.numel() != graph.E:
            raise _l.VglHipError("quotient_graph: %d weights for %d entries" % (w.numel(), graph.E))
        w = w.to(torch.int64).contiguous() if graph.E else torch.zeros(1, dtype=torch.int64, device=ctx.device)
    plan = C.c_void_p()
    _l.check(ctx.L.vgl_hip_quotient_plan_create(ctx.h, graph.h, _ptr(lab), int(not self_loops), C.byref(plan)))
    try:
        vc, eo, ei, st = C.c_int32(), C.c_int64(), C.c_int64(), _l.QuotientStats()
        _l.check(ctx.L.vgl_hip_quotient_plan_info(plan, C.byref(vc), C.byref(eo), C.byref(ei), C.byref(st)))
        vc, eo, ei = vc.value, eo.value, ei.value
        cluster_of, label_of, size = ctx.empty(graph.V, torch.int32), ctx.empty(vc, torch.int32), ctx.empty(vc, torch.int32)
        _l.check(ctx.L.vgl_hip_quotient_plan_vertex_maps(ctx.h, plan, _ptr(cluster_of), _ptr(label_of), _ptr(size)))
        rowptr, adj, count = ctx.empty(vc + 1, torch.int64), ctx.empty(max(eo, 1), torch.int32), ctx.empty(max(eo, 1), torch.int64)
        _l.check(ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 0, _ptr(w), _ptr(rowptr), _ptr(adj), _ptr(count)))
        adj, count = adj[:eo], count[:eo]
        in_rowptr = in_adj = in_count = None
        if want_in and w is None and ei >= 0:
            in_rowptr, in_adj, in_count = ctx.empty(vc + 1, torch.int64), ctx.empty(max(ei, 1), torch.int32), ctx.empty(max(ei, 1), torch.int64)
            _l.check(ctx.L.vgl_hip_quotient_plan_fill(ctx.h, plan, 1, None, _ptr(in_rowptr), _ptr(in_adj), _ptr(in_count)))
            in_adj, in_count = in_adj[:ei], in_count[:ei]
        elif want_in:                                                 # the transposition of Graph.from_coo; the counts follow its permutation
            csr_src = torch.repeat_interleave(torch.arange(vc, device=ctx.device, dtype=torch.int32), rowptr[1:] - rowptr[:-1])
            in_rowptr, in_adj, perm = ctx.coo_to_csr(vc, adj, csr_src, want_perm=True)
            in_count = count[perm]
        ctx.sync()                                                    # the fills read the plan's arrays
    finally:
        ctx.L.vgl_hip_quotient_plan_destroy(ctx.h, plan)
    q = Graph(ctx, vc, rowptr, adj, in_rowptr, in_adj)
    q.count, q.in_count, q.label_of, q.size = count, in_count, label_of, size
    q.cluster_of = cluster_of if raw else graph.to_original(cluster_of)
    q.stats = _stats(st)
    return q


def partition_quality(graph, labels, weights=None, raw=False):
    """how good a partition is, derived from quotient_graph() in torch (no further kernel).  Returns a dict: label_of (int32 [V']), size (int32 [V']),
    internal (int64 [V'], the diagonal counts: the weight of the stored entries inside the cluster), volume_out / volume_in (int64 [V'], the weight of
    the stored entries that leave / enter the cluster's vertices, the internal ones included), total (m, the weight of all stored entries),
    cut = m - sum(internal) and coverage = sum(internal) / m (1.0 for m = 0) as a Python int, int and float, and
    modularity = sum over c of (internal_c / m - volume_out_c * volume_in_c / m^2) in float64, 0.0 for m = 0.  On a graph that stores both directions
    of every edge this is Newman's undirected modularity with 2m = the stored total; on a directed graph it is the directed modularity of Leicht
    and Newman."""
    q = quotient_graph(graph, labels, weights=weights, self_loops=True, raw=raw)
    dev = graph.ctx.device
    vc = q.V
    rows = torch.repeat_interleave(torch.arange(vc, device=dev), q.out_rowptr[1:] - q.out_rowptr[:-1])
    cols = q.out_adj.long()
    zeros = torch.zeros(vc, dtype=torch.int64, device=dev)
    internal = zeros.clone().index_add_(0, rows, torch.where(rows == cols, q.count, torch.zeros_like(q.count)))
    volume_out = zeros.clone().index_add_(0, rows, q.count)
    if q.in_rowptr is not None:
        in_rows = torch.repeat_interleave(torch.arange(vc, device=dev), q.in_rowptr[1:] - q.in_rowptr[:-1])
        volume_in = zeros.clone().index_add_(0, in_rows, q.in_count)
    else:
        volume_in = zeros.clone().index_add_(0, cols, q.count)
    m = int(volume_out.sum())
    inside = int(internal.sum())
    if m == 0:
        mod = 0.0
    else:
        mod = float((internal.double() / m - volume_out.double() * volume_in.double() / (float(m) * float(m))).sum())
    return {"label_of": q.label_of, "size": q.size, "internal": internal, "volume_out": volume_out, "volume_in": volume_in, "total": m,
            "cut": m - inside, "coverage": (inside / m) if m else 1.0, "modularity": mod}


def modularity(graph, labels, weights=None, raw=False):
    """the modularity of a partition: partition_quality(...)["modularity"]"""
    return partition_quality(graph, labels, weights=weights, raw=raw)["modularity"]


def condensation(graph, raw=False):
    """the condensation of a directed graph: quotient_graph() by the labels of strongly_connected_components() with self_loops=False -- one vertex per
    strongly connected component, acyclic.  dag.cluster_of maps every vertex (ORIGINAL order unless raw=True) to its component's vertex."""
    comp, _ = strongly_connected_components(graph, raw=raw)
    return quotient_graph(graph, comp, self_loops=False, raw=raw)


LOUVAIN_OUTCOMES = ("converged", "reverted", "small_gain", "capped")


def _louvain_weights(graph, weights, who):
    if weights is None:
        return None
    w = torch.as_tensor(weights).to(graph.ctx.device).flatten()
    if w.is_floating_point() or w.dtype == torch.bool:
        raise _l.VglHipError(who + ": weights must be integers")
    if w.numel() != graph.E:
        raise _l.VglHipError("%s: %d weights for %d entries" % (who, w.numel(), graph.E))
    return w.to(torch.int64).contiguous() if graph.E else torch.zeros(1, dtype=torch.int64, device=graph.ctx.device)


def _louvain_info(st):
    n = int(st.levels)
    info = {k: getattr(st, k) for k, t in st._fields_ if not issubclass(t, C.Array)}
    for k, t in st._fields_:
        if issubclass(t, C.Array):
            info[k] = [int(x) for x in getattr(st, k)[:n]]
    info["outcome"] = [LOUVAIN_OUTCOMES[x] for x in info["outcome"]]
    m = int(st.total_weight)
    info["modularity"] = (int(st.modularity_num) / (m * m)) if m else 0.0
    return info


def louvain_move(graph, weights=None, max_rounds=64, min_gain_den=0, seed=0, raw=False):
    """one level of move rounds on the stored outgoing CSR as it is (the contract of vgl_hip_louvain_move; the caller vouches that it is symmetric;
    repeats and loops allowed).  weights: int64 per stored entry, None = 1 each.  Returns (labels, info): labels int32 [V], the ORIGINAL id of the
    vertex that names the community, in ORIGINAL vertex order (own ids and own order with raw=True)."""
    ctx = graph.ctx
    w = _louvain_weights(graph, weights, "louvain_move")
    label = ctx.empty(max(graph.V, 1), torch.int32)[:graph.V]
    st = _l.LouvainStats()
    _l.check(ctx.L.vgl_hip_louvain_move(ctx.h, graph.h, _ptr(w), int(max_rounds), int(min_gain_den), int(seed) & 0xFFFFFFFF, _ptr(label), C.byref(st)))
    info = _louvain_info(st)
    if not raw and graph.fwd is not None:
        label = graph.to_original(graph.bwd[label.long()].to(torch.int32).contiguous())
    return label, info


def count_not_equal(ctx, a, b):
    r = C.c_int64()
    _l.check(ctx.L.vgl_hip_count_not_equal_u32(ctx.h, a.numel(), _ptr(a), _ptr(b), C.byref(r)))
    return r.value


# ---- neighbour aggregation with gradients (the contract of vgl_hip_agg_* in include/vgl_hip.h) ----
AGG_OPS = {"sum": 0, "mean": 1, "max": 2, "min": 3}


def _agg_stats(st):
    d = {k: getattr(st, k) for k, _ in st._fields_ if k != "column_tiles"}
    d["column_tiles"] = list(st.column_tiles)
    return d


class AggregationPlan:
    """A device CSR (rowptr int64 [n_rows + 1], adj int32 [E] with entries in [0, n_cols)) prepared for aggregate(): checked, its rows classified and
    chunked once; the transpose that the backward pass walks is built by the first backward and kept.  The plan BORROWS the two tensors (it keeps a
    reference, they must not be modified).  Entries are taken as stored: repeats count, self entries are entries.  last_stats / last_backward_stats
    hold the stats of the latest forward / backward run."""

    def __init__(self, ctx, rowptr, adj, n_cols):
        if rowptr.dtype != torch.int64 or adj.dtype != torch.int32:
            raise _l.VglHipError("AggregationPlan: rowptr must be int64 and adj int32, got %s and %s" % (rowptr.dtype, adj.dtype))
        if rowptr.dim() != 1 or rowptr.numel() < 1 or adj.dim() != 1:
            raise _l.VglHipError("AggregationPlan: rowptr must hold n_rows + 1 offsets and adj be one-dimensional")
        if rowptr.device != ctx.device or adj.device != ctx.device:
            raise _l.VglHipError("AggregationPlan: rowptr and adj must live on the context's device")
        self.ctx, self.rowptr, self.adj = ctx, rowptr.contiguous(), adj.contiguous()
        self.n_rows, self.n_cols, self.E = int(rowptr.numel()) - 1, int(n_cols), int(adj.numel())
        if int(self.rowptr[-1]) != self.E:
            raise _l.VglHipError("AggregationPlan: rowptr ends at %d but adj has %d entries" % (int(self.rowptr[-1]), self.E))
        self.last_stats = self.last_backward_stats = self.last_edge_stats = None
        h = C.c_void_p()
        keep = self.adj if self.E else ctx.empty(1, torch.int32)
        _l.check(ctx.L.vgl_hip_agg_plan_create(ctx.h, _ptr(self.rowptr), _ptr(keep), self.n_rows, self.n_cols, C.byref(h)))
        self.h = h

    @classmethod
    def from_graph(cls, graph, direction="in"):
        """the stored CSR of `direction` in the graph's OWN numbering: n_rows = n_cols = V, row v aggregates over the incoming ("in") or outgoing
        ("out") entries of v"""
        if direction not in ("in", "out"):
            raise _l.VglHipError("AggregationPlan.from_graph: direction must be 'in' or 'out'")
        rowptr, adj = (graph.in_rowptr, graph.in_adj) if direction == "in" else (graph.out_rowptr, graph.out_adj)
        if rowptr is None:
            raise _l.VglHipError("AggregationPlan.from_graph: the graph has no incoming CSR")
        if graph.row_begin != 0 or graph.row_end != graph.V:
            raise _l.VglHipError("AggregationPlan.from_graph: graph handle must own all rows")
        return cls(graph.ctx, rowptr, adj, graph.V)

    @classmethod
    def from_block(cls, ctx, block):
        """a dict of sample_blocks -> (plan, cols): cols is the sorted unique union of the block's seeds and samples (what sample_blocks takes as its
        next frontier when its ids are the graph's own: raw=True or no renumbering), the plan's adj the position of each sample in cols: row i of the
        block aggregates rows of a len(cols) x F input"""
        seeds, adj = block["seeds"], block["adj"]
        cols = torch.unique(torch.cat([seeds, adj])).to(torch.int32).contiguous()
        pos = torch.searchsorted(cols, adj).to(torch.int32).contiguous()
        return cls(ctx, block["rowptr"], pos, int(cols.numel())), cols

    def info(self):
        st = _l.AggStats()
        _l.check(self.ctx.L.vgl_hip_agg_plan_info(self.h, C.byref(st)))
        return _agg_stats(st)

    def close(self):
        if self.h:
            self.ctx.L.vgl_hip_agg_plan_destroy(self.ctx.h, self.h)
            self.h = None

    @staticmethod
    def _rows(t, who):
        """(tensor to pass, leading dimension): a view whose rows are strided by elements goes as it is"""
        if t.dim() != 2:
            raise _l.VglHipError("%s must be two-dimensional (rows x F)" % who)
        F = int(t.shape[1])
        if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < F):
            t = t.contiguous()
        elif t.shape[0] <= 1 and t.stride(1) != 1:
            t = t.contiguous()
        return t, (int(t.stride(0)) if t.shape[0] > 1 else F)

    def _forward(self, x, op, weight):
        ctx, F = self.ctx, int(x.shape[1])
        ext = op >= 2
        out = torch.empty((self.n_rows, F), dtype=torch.float32, device=ctx.device)
        arg = torch.empty((self.n_rows, F), dtype=torch.int32, device=ctx.device) if ext else None
        if self.n_rows == 0 or F == 0:
            return out, arg
        if self.n_cols == 0:
            return out.zero_(), (arg.fill_(-1) if ext else None)
        x, ldx = self._rows(x, "aggregate: x")
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_run(ctx.h, self.h, op, _ptr(weight), _ptr(x), ldx, F, _ptr(out), F, _ptr(arg), C.byref(st)))
        self.last_stats = _agg_stats(st)
        return out, arg

    def _backward(self, g, op, weight, arg):
        ctx, F = self.ctx, int(g.shape[1])
        gx = torch.empty((self.n_cols, F), dtype=torch.float32, device=ctx.device)
        if self.n_cols == 0 or F == 0:
            return gx
        if self.n_rows == 0:
            return gx.zero_()
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_run_transposed(ctx.h, self.h, op, _ptr(weight), _ptr(arg), _ptr(g), F, F, _ptr(gx), F, C.byref(st)))
        self.last_backward_stats = _agg_stats(st)
        return gx

    # one float32 per entry (vgl_hip_agg_sddmm / _edge_softmax in include/vgl_hip.h); last_edge_stats: the stats of the latest call
    def _sddmm(self, a, b, mean=0):
        ctx, F = self.ctx, int(a.shape[1])
        e = torch.empty(self.E, dtype=torch.float32, device=ctx.device)
        if self.E == 0:
            return e
        if F == 0:
            return e.zero_()
        a, lda = self._rows(a, "sddmm: a")
        b, ldb = self._rows(b, "sddmm: b")
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_sddmm(ctx.h, self.h, _ptr(a), lda, _ptr(b), ldb, F, int(mean), _ptr(e), C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return e

    def _edge_softmax(self, e):
        y = torch.empty(self.E, dtype=torch.float32, device=self.ctx.device)
        if self.E == 0:
            return y
        st = _l.AggStats()
        _l.check(self.ctx.L.vgl_hip_agg_edge_softmax(self.ctx.h, self.h, _ptr(e), _ptr(y), C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return y

    def _edge_softmax_backward(self, y, gy):
        ge = torch.empty(self.E, dtype=torch.float32, device=self.ctx.device)
        if self.E == 0:
            return ge
        st = _l.AggStats()
        _l.check(self.ctx.L.vgl_hip_agg_edge_softmax_backward(self.ctx.h, self.h, _ptr(y), _ptr(gy), _ptr(ge), C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return ge

    # H heads in one walk (the vgl_hip_agg_*_heads calls): the edge scalars are E x H contiguous, head h owns F / H columns
    def _forward_heads(self, x, op, weight, H):
        ctx, F = self.ctx, int(x.shape[1])
        out = torch.empty((self.n_rows, F), dtype=torch.float32, device=ctx.device)
        if self.n_rows == 0 or F == 0:
            return out
        if self.n_cols == 0 or self.E == 0:
            return out.zero_()
        x, ldx = self._rows(x, "spmm: x")
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_run_heads(ctx.h, self.h, op, _ptr(weight), H, _ptr(x), ldx, F, _ptr(out), F, C.byref(st)))
        self.last_stats = _agg_stats(st)
        return out

    def _backward_heads(self, g, op, weight, H):
        ctx, F = self.ctx, int(g.shape[1])
        gx = torch.empty((self.n_cols, F), dtype=torch.float32, device=ctx.device)
        if self.n_cols == 0 or F == 0:
            return gx
        if self.n_rows == 0 or self.E == 0:
            return gx.zero_()
        g, ldg = self._rows(g, "spmm: grad")
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_run_transposed_heads(ctx.h, self.h, op, _ptr(weight), H, _ptr(g), ldg, F, _ptr(gx), F, C.byref(st)))
        self.last_backward_stats = _agg_stats(st)
        return gx

    def _sddmm_heads(self, a, b, H, mean=0):
        ctx, F = self.ctx, int(a.shape[1])
        e = torch.empty((self.E, H), dtype=torch.float32, device=ctx.device)
        if self.E == 0:
            return e
        if F == 0:
            return e.zero_()
        a, lda = self._rows(a, "sddmm: a")
        b, ldb = self._rows(b, "sddmm: b")
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_sddmm_heads(ctx.h, self.h, _ptr(a), lda, _ptr(b), ldb, F, H, int(mean), _ptr(e), C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return e

    def _edge_softmax_heads(self, e):
        H = int(e.shape[1])
        y = torch.empty((self.E, H), dtype=torch.float32, device=self.ctx.device)
        if self.E == 0 or H == 0:
            return y
        st = _l.AggStats()
        _l.check(self.ctx.L.vgl_hip_agg_edge_softmax_heads(self.ctx.h, self.h, _ptr(e), H, _ptr(y), C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return y

    def _edge_softmax_backward_heads(self, y, gy):
        H = int(y.shape[1])
        ge = torch.empty((self.E, H), dtype=torch.float32, device=self.ctx.device)
        if self.E == 0 or H == 0:
            return ge
        st = _l.AggStats()
        _l.check(self.ctx.L.vgl_hip_agg_edge_softmax_backward_heads(self.ctx.h, self.h, _ptr(y), _ptr(gy), H, _ptr(ge), C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return ge

    # the additive score and the entry sums (vgl_hip_agg_edge_add_heads / _edge_sum_heads); s or t None: the term is absent
    def _edge_add(self, s, t, H, slope):
        ctx = self.ctx
        e = torch.empty((self.E, H), dtype=torch.float32, device=ctx.device)
        if self.E == 0 or H == 0:
            return e
        s, lds = self._rows(s, "u_add_v: s") if s is not None else (None, 0)
        t, ldt = self._rows(t, "u_add_v: t") if t is not None else (None, 0)
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_edge_add_heads(ctx.h, self.h, _ptr(s), lds, _ptr(t), ldt, H, float(slope), _ptr(e), C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return e

    def _edge_sum(self, w, gate, slope, transposed):
        ctx, H = self.ctx, int(w.shape[1])
        out = torch.empty((self.n_cols if transposed else self.n_rows, H), dtype=torch.float32, device=ctx.device)
        if out.numel() == 0:
            return out
        if self.E == 0:
            return out.zero_()
        st = _l.AggStats()
        _l.check(ctx.L.vgl_hip_agg_edge_sum_heads(ctx.h, self.h, _ptr(w), _ptr(gate), float(slope), H, 1 if transposed else 0, _ptr(out), H, C.byref(st)))
        self.last_edge_stats = _agg_stats(st)
        return out


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(fctx, x, plan, op, weight):
        out, arg = plan._forward(x.detach(), op, weight)
        fctx.plan, fctx.op = plan, op
        fctx.save_for_backward(weight, arg)
        if arg is not None:
            fctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(fctx, grad_out, _grad_arg=None):
        weight, arg = fctx.saved_tensors
        return fctx.plan._backward(grad_out.contiguous(), fctx.op, weight, arg), None, None, None


def aggregate(plan, x, op="sum", weight=None, return_arg=False):
    """out[i, :] = the sum / mean / max / min over the entries p of row i of the plan of x[adj[p], :] (x: n_cols x F float32 on the plan's device;
    weight: one float32 per entry in CSR order, sum and mean only).  Returns out (n_rows x F), and with return_arg=True also arg (int32, n_rows x F: the
    smallest position that attains the extreme, -1 in an empty row; None for sum and mean).  An empty row gives 0.  Differentiable in x ONLY: backward
    runs the transposed kernel on grad_out.contiguous(), without atomics, so gradients are the same bits on every run; a weight that requires grad is
    refused.  x may be a column slice or an offset view: a view whose rows are strided by elements is passed with its leading dimension, anything
    else is made contiguous first.  The pinned counter mirror is per context, so run ONE aggregate (forward or backward) at a time per context."""
    if not isinstance(plan, AggregationPlan) or not plan.h:
        raise _l.VglHipError("aggregate: plan must be an open AggregationPlan")
    if op not in AGG_OPS:
        raise _l.VglHipError("aggregate: op must be one of 'sum', 'mean', 'max', 'min', got %r" % (op,))
    if not torch.is_tensor(x) or x.dtype != torch.float32:
        raise _l.VglHipError("aggregate: x must be a float32 tensor, got %s" % (x.dtype if torch.is_tensor(x) else type(x).__name__))
    if x.dim() != 2 or int(x.shape[0]) != plan.n_cols:
        raise _l.VglHipError("aggregate: x must be n_cols x F = %d x F, got %s" % (plan.n_cols, tuple(x.shape)))
    if x.device != plan.ctx.device:
        raise _l.VglHipError("aggregate: x must live on the plan's device")
    if weight is not None:
        if op in ("max", "min"):
            raise _l.VglHipError("aggregate: max and min take no entry weights")
        if not torch.is_tensor(weight) or weight.dtype != torch.float32:
            raise _l.VglHipError("aggregate: weight must be a float32 tensor, got %s" % (weight.dtype if torch.is_tensor(weight) else type(weight).__name__))
        if weight.requires_grad:
            raise _l.VglHipError("aggregate: differentiable in x only; for gradients with respect to entry weights (SDDMM) call api.spmm, or pass weight.detach()")
        if weight.dim() != 1 or int(weight.numel()) != plan.E or weight.device != plan.ctx.device:
            raise _l.VglHipError("aggregate: weight must hold one value per entry (%d) on the plan's device" % plan.E)
        weight = weight.contiguous()
    out, arg = _Aggregate.apply(x, plan, AGG_OPS[op], weight)
    return (out, arg) if return_arg else out


def aggregate_neighbors(graph, x, op="sum", weight=None, direction="in", raw=False):
    """aggregate() over the stored CSR of `direction`: x (V x F float32) and the result are in ORIGINAL vertex order unless raw=True; weight is per
    entry of the graph's stored in_adj / out_adj.  On a renumbered graph this pays one row permutation of x and one of the result; raw=True pays
    neither.  The plan is cached on the Graph per direction and closed with it."""
    plans = graph.__dict__.setdefault("_agg_plans", {})
    if direction not in plans:
        plans[direction] = AggregationPlan.from_graph(graph, direction)
    permute = not raw and graph.fwd is not None
    if permute:
        x = x[graph.bwd.long()]
    out = aggregate(plans[direction], x, op, weight)
    return out[graph.fwd.long()] if permute else out


# ---- edge scores, edge softmax and graph attention (the contract of vgl_hip_agg_sddmm / _edge_softmax in include/vgl_hip.h) ----
def _edge_plan(who, plan):
    if not isinstance(plan, AggregationPlan) or not plan.h:
        raise _l.VglHipError("%s: plan must be an open AggregationPlan" % who)


def _edge_features(who, name, plan, t, rows, what):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise _l.VglHipError("%s: %s must be a float32 tensor, got %s" % (who, name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() != 2 or int(t.shape[0]) != rows:
        raise _l.VglHipError("%s: %s must be %s x F = %d x F, got %s" % (who, name, what, rows, tuple(t.shape)))
    if t.device != plan.ctx.device:
        raise _l.VglHipError("%s: %s must live on the plan's device" % (who, name))


def _edge_scalars(who, name, plan, t):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise _l.VglHipError("%s: %s must be a float32 tensor, got %s" % (who, name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() != 1 or int(t.numel()) != plan.E or t.device != plan.ctx.device:
        raise _l.VglHipError("%s: %s must hold one value per entry (%d) on the plan's device" % (who, name, plan.E))


class _Sddmm(torch.autograd.Function):
    @staticmethod
    def forward(fctx, a, b, plan):
        fctx.plan = plan
        fctx.save_for_backward(a, b)
        return plan._sddmm(a.detach(), b.detach(), 0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, ge):
        a, b = fctx.saved_tensors
        ge = ge.contiguous()
        # the two existing runs with the entry gradient as the weight: ga[i] = sum_p ge[p] b[adj[p]], gb[u] = sum over adj[p] = u of ge[p] a[row(p)]
        ga = fctx.plan._forward(b, AGG_OPS["sum"], ge)[0] if fctx.needs_input_grad[0] else None
        gb = fctx.plan._backward(a.contiguous(), AGG_OPS["sum"], ge, None) if fctx.needs_input_grad[1] else None
        return ga, gb, None


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(fctx, e, plan):
        y = plan._edge_softmax(e.detach().contiguous())
        fctx.plan = plan
        fctx.save_for_backward(y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gy):
        (y,) = fctx.saved_tensors
        return fctx.plan._edge_softmax_backward(y, gy.contiguous()), None


class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(fctx, weight, x, plan, op):
        fctx.plan, fctx.op = plan, op
        fctx.save_for_backward(weight, x)
        return plan._forward(x.detach(), op, weight.detach())[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, g):
        weight, x = fctx.saved_tensors
        g = g.contiguous()
        gw = fctx.plan._sddmm(g, x, 1 if fctx.op == AGG_OPS["mean"] else 0) if fctx.needs_input_grad[0] else None
        gx = fctx.plan._backward(g, fctx.op, weight, None) if fctx.needs_input_grad[1] else None
        return gw, gx, None, None


# ---- heads: E x H scalars, head h owns F / H columns (the vgl_hip_agg_*_heads calls in include/vgl_hip.h) ----
def _edge_heads(who, heads):
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise _l.VglHipError("%s: heads must be an int of at least 1, got %r" % (who, heads))
    return heads


def _edge_scalars_heads(who, name, plan, t):
    """(E,) or (E, H) float32 on the plan's device -> H, or None for (E,)"""
    if torch.is_tensor(t) and t.dim() == 2:
        if t.dtype != torch.float32:
            raise _l.VglHipError("%s: %s must be a float32 tensor, got %s" % (who, name, t.dtype))
        if int(t.shape[0]) != plan.E or int(t.shape[1]) < 1 or t.device != plan.ctx.device:
            raise _l.VglHipError("%s: %s must hold one value per entry (%d), or per entry and head (%d x H, H >= 1), on the plan's device" % (who, name, plan.E, plan.E))
        return int(t.shape[1])
    _edge_scalars(who, name, plan, t)
    return None


class _SddmmHeads(torch.autograd.Function):
    @staticmethod
    def forward(fctx, a, b, plan, H):
        fctx.plan, fctx.H = plan, H
        fctx.save_for_backward(a, b)
        return plan._sddmm_heads(a.detach(), b.detach(), H, 0)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, ge):
        a, b = fctx.saved_tensors
        ge = ge.contiguous()
        # the two heads runs with the E x H entry gradient as the weight
        ga = fctx.plan._forward_heads(b, AGG_OPS["sum"], ge, fctx.H) if fctx.needs_input_grad[0] else None
        gb = fctx.plan._backward_heads(a, AGG_OPS["sum"], ge, fctx.H) if fctx.needs_input_grad[1] else None
        return ga, gb, None, None


class _EdgeSoftmaxHeads(torch.autograd.Function):
    @staticmethod
    def forward(fctx, e, plan):
        y = plan._edge_softmax_heads(e.detach().contiguous())
        fctx.plan = plan
        fctx.save_for_backward(y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, gy):
        (y,) = fctx.saved_tensors
        return fctx.plan._edge_softmax_backward_heads(y, gy.contiguous()), None


class _SpmmHeads(torch.autograd.Function):
    @staticmethod
    def forward(fctx, weight, x, plan, op):
        fctx.plan, fctx.op, fctx.H = plan, op, int(weight.shape[1])
        fctx.save_for_backward(weight, x)
        return plan._forward_heads(x.detach(), op, weight.detach(), fctx.H)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, g):
        weight, x = fctx.saved_tensors
        g = g.contiguous()
        gw = fctx.plan._sddmm_heads(g, x, fctx.H, 1 if fctx.op == AGG_OPS["mean"] else 0) if fctx.needs_input_grad[0] else None
        gx = fctx.plan._backward_heads(g, fctx.op, weight, fctx.H) if fctx.needs_input_grad[1] else None
        return gw, gx, None, None


def sddmm(plan, a, b, heads=None):
    """e[p] = the dot product of a[row(p), :] and b[adj[p], :] for every stored entry p of the plan, in CSR order (a: n_rows x F, b: n_cols x F, float32
    on the plan's device) -> E float32.  With heads=H (an int that divides F) head h owns the columns [h F / H, (h + 1) F / H) and the result is
    E x H: e[p, h] = the dot product over the columns of head h, every head in one walk of the plan, each column with the bits of the call on the
    head's column slice.  Differentiable in a and b, first order: the backward is aggregate's forward kernel (grad a) and its transposed kernel
    (grad b) with the entry gradient as the weight, without atomics, the same bits on every run.  Column slices and offset views go with their
    leading dimension.  One call at a time per context."""
    _edge_plan("sddmm", plan)
    _edge_features("sddmm", "a", plan, a, plan.n_rows, "n_rows")
    _edge_features("sddmm", "b", plan, b, plan.n_cols, "n_cols")
    if int(a.shape[1]) != int(b.shape[1]):
        raise _l.VglHipError("sddmm: a and b must have the same width F, got %d and %d" % (int(a.shape[1]), int(b.shape[1])))
    if heads is None:
        return _Sddmm.apply(a, b, plan)
    H = _edge_heads("sddmm", heads)
    if int(a.shape[1]) % H != 0:
        raise _l.VglHipError("sddmm: the width F = %d must be divisible by heads = %d" % (int(a.shape[1]), H))
    return _SddmmHeads.apply(a, b, plan, H)


def edge_softmax(plan, e):
    """y[p] = exp(e[p] - m) / s over the entries of each row of the plan (m the row's largest score, s the sum; one division per entry) -> E float32.
    e may also be E x H (one column per head, H >= 2; E x 1 is refused as it always was: one head is (E,)): the softmax of every (row, head), each
    column with the bits of the call on that column -> E x H.
    An entry at -inf gets 0, a row of -inf alone 0 everywhere; with NaN or +inf the result is unspecified.  Differentiable, first order:
    ge[p] = y[p] * (gy[p] - sum_q y[q] gy[q])."""
    _edge_plan("edge_softmax", plan)
    if torch.is_tensor(e) and e.dim() == 2 and int(e.shape[1]) == 1:
        # E x 1 stays refused, as it was before heads existed: one head is (E,); graph_attention(heads=1) keeps its E x 1 scores to itself
        _edge_scalars("edge_softmax", "e", plan, e)
    return _edge_softmax_any(plan, e)


def _edge_softmax_any(plan, e):
    if _edge_scalars_heads("edge_softmax", "e", plan, e) is None:
        return _EdgeSoftmax.apply(e, plan)
    return _EdgeSoftmaxHeads.apply(e, plan)


def spmm(plan, weight, x, op="sum"):
    """aggregate(plan, x, op, weight) for op "sum" or "mean", differentiable in BOTH weight (one float32 per entry) and x (n_cols x F): grad x is the
    transposed run, grad weight[p] = the dot product of grad_out[row(p), :] and x[adj[p], :] (divided by the row's length for "mean"), first order.
    weight may also be E x H with F divisible by H: column h weighs the columns [h F / H, (h + 1) F / H) of x, and grad weight is E x H."""
    _edge_plan("spmm", plan)
    if op not in ("sum", "mean"):
        raise _l.VglHipError("spmm: op must be 'sum' or 'mean', got %r" % (op,))
    H = _edge_scalars_heads("spmm", "weight", plan, weight)
    _edge_features("spmm", "x", plan, x, plan.n_cols, "n_cols")
    if H is None:
        return _Spmm.apply(weight.contiguous(), x, plan, AGG_OPS[op])
    if int(x.shape[1]) % H != 0:
        raise _l.VglHipError("spmm: the width F = %d of x must be divisible by the heads of weight (%d)" % (int(x.shape[1]), H))
    return _SpmmHeads.apply(weight.contiguous(), x, plan, AGG_OPS[op])


def graph_attention(plan, q, k, v, scale=None, return_weights=False, heads=None):
    """out[i, :] = sum over the entries p of row i of softmax_row(scale * q[i] . k[adj[p]])[p] * v[adj[p], :]: dot-product attention of every row over
    its stored entries (q: n_rows x F, k: n_cols x F, v: n_cols x Fv; scale F ** -0.5 unless given).  It IS spmm(plan, edge_softmax(plan, sddmm(plan,
    q, k) * scale), v) and nothing else, so it is differentiable in q, k and v.  With heads=H (H divides F and Fv) every head attends on its own
    columns in the same three calls: spmm(plan, edge_softmax(plan, sddmm(plan, q, k, heads=H) * scale), v) with scale (F / H) ** -0.5 unless given,
    head h of out in the columns [h Fv / H, (h + 1) Fv / H).  With return_weights=True also the attention weights: E, with heads E x H."""
    if heads is None:
        e = sddmm(plan, q, k)
        if scale is None:
            scale = float(q.shape[1]) ** -0.5 if int(q.shape[1]) > 0 else 1.0
    else:
        H = _edge_heads("graph_attention", heads)
        _edge_features("graph_attention", "v", plan, v, plan.n_cols, "n_cols")
        if int(v.shape[1]) % H != 0:
            raise _l.VglHipError("graph_attention: the width %d of v must be divisible by heads = %d" % (int(v.shape[1]), H))
        e = sddmm(plan, q, k, heads=H)
        if scale is None:
            scale = float(int(q.shape[1]) // H) ** -0.5 if int(q.shape[1]) > 0 else 1.0
    w = edge_softmax(plan, e * scale) if heads is None else _edge_softmax_any(plan, e * scale)
    out = spmm(plan, w, v)
    return (out, w) if return_weights else out


# ---- the additive score of GAT, the entry sums and GAT attention (vgl_hip_agg_edge_add_heads / _edge_sum_heads in include/vgl_hip.h) ----
def _gat_slope(who, negative_slope):
    """(slope, gated): None is the identity"""
    if negative_slope is None:
        return 1.0, False
    if isinstance(negative_slope, bool) or not isinstance(negative_slope, (int, float)) or not 0.0 <= float(negative_slope) < float("inf"):
        raise _l.VglHipError("%s: negative_slope must be None or a finite number that is not negative, got %r" % (who, negative_slope))
    return float(negative_slope), True


def _gat_term(who, name, plan, t, rows, what):
    """(n,) or (n, H) float32 on the plan's device -> the n x H view, and whether it was one-dimensional"""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise _l.VglHipError("%s: %s must be a float32 tensor, got %s" % (who, name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() not in (1, 2) or int(t.shape[0]) != rows:
        raise _l.VglHipError("%s: %s must be (%s,) or %s x H = %d [x H], got %s" % (who, name, what, what, rows, tuple(t.shape)))
    if t.device != plan.ctx.device:
        raise _l.VglHipError("%s: %s must live on the plan's device" % (who, name))
    return (t.unsqueeze(1), True) if t.dim() == 1 else (t, False)


class _UAddV(torch.autograd.Function):
    @staticmethod
    def forward(fctx, s, t, plan, slope, gated):
        e = plan._edge_add(s.detach(), t.detach(), int(s.shape[1]), slope)
        fctx.plan, fctx.slope, fctx.gated = plan, slope, gated
        if gated:
            fctx.save_for_backward(e)
        return e

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, ge):
        gate = fctx.saved_tensors[0] if fctx.gated else None              # slope >= 0: the score has the sign of the sum, it is its own gate
        ge = ge.contiguous()
        gs = fctx.plan._edge_sum(ge, gate, fctx.slope, False) if fctx.needs_input_grad[0] else None
        gt = fctx.plan._edge_sum(ge, gate, fctx.slope, True) if fctx.needs_input_grad[1] else None
        return gs, gt, None, None, None


class _EdgeSum(torch.autograd.Function):
    @staticmethod
    def forward(fctx, w, plan, transposed):
        fctx.plan, fctx.transposed = plan, transposed
        return plan._edge_sum(w.detach().contiguous(), None, 1.0, transposed)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, g):
        # the broadcast of g onto the entries: the score with one term absent and slope 1
        H = int(g.shape[1])
        return (fctx.plan._edge_add(None, g, H, 1.0) if fctx.transposed else fctx.plan._edge_add(g, None, H, 1.0)), None, None


def u_add_v(plan, s, t, negative_slope=None):
    """e[p] = act(s[row(p)] + t[adj[p]]) for every stored entry p of the plan, in CSR order: the additive score of the original GAT.  s is (n_rows,)
    and t (n_cols,), float32 on the plan's device -> (E,); or s is n_rows x H and t n_cols x H -> E x H, every head in one walk.  act is LeakyReLU
    with negative_slope (z > 0 ? z : negative_slope * z, one float32 product after one float32 addition; 0 is ReLU); None is the identity.  The
    result equals the float32 formula bit for bit.  Differentiable in s and t, first order: grad s[i] = the sum over the entries of row i of the
    gated entry gradient, grad t[u] the same sum over the entries with adj[p] = u in ascending p (the saved score is the gate), both without atomics:
    the same bits on every run.  Column slices and offset views go with their leading dimension.  One call at a time per context."""
    _edge_plan("u_add_v", plan)
    slope, gated = _gat_slope("u_add_v", negative_slope)
    s2, s_flat = _gat_term("u_add_v", "s", plan, s, plan.n_rows, "n_rows")
    t2, t_flat = _gat_term("u_add_v", "t", plan, t, plan.n_cols, "n_cols")
    if s_flat != t_flat or int(s2.shape[1]) != int(t2.shape[1]):
        raise _l.VglHipError("u_add_v: s and t must both be one-dimensional or have the same number of heads, got %s and %s" % (tuple(s.shape), tuple(t.shape)))
    e = _UAddV.apply(s2, t2, plan, slope, gated)
    return e.squeeze(1) if s_flat else e


def edge_sum(plan, w, transposed=False):
    """out[i] = the sum of w[p] over the entries p of row i of the plan (w: (E,) or E x H float32 -> (n_rows,) or n_rows x H); with transposed=True
    out[u] = the sum over the entries with adj[p] = u, in ascending p -> (n_cols,) or n_cols x H.  An empty row or column gives 0.  No atomics: the
    same bits on every run.  Differentiable, first order: the gradient of w[p] is grad_out[row(p)], or grad_out[adj[p]] when transposed."""
    _edge_plan("edge_sum", plan)
    if not isinstance(transposed, (bool, int)) or transposed not in (0, 1):
        raise _l.VglHipError("edge_sum: transposed must be True or False, got %r" % (transposed,))
    if _edge_scalars_heads("edge_sum", "w", plan, w) is None:
        return _EdgeSum.apply(w.unsqueeze(1), plan, bool(transposed)).squeeze(1)
    return _EdgeSum.apply(w, plan, bool(transposed))


def gat_attention(plan, s, t, v, negative_slope=0.2, return_weights=False):
    """out[i, :] = the sum over the entries p of row i of softmax_row(leaky_relu(s[i] + t[adj[p]]))[p] * v[adj[p], :]: the attention of the original
    GAT layer, given the two projections of the features on the attention vector (s: n_rows x H, t: n_cols x H, v: n_cols x Fv with Fv divisible by
    H; head h of out in the columns [h Fv / H, (h + 1) Fv / H)).  It IS spmm(plan, edge_softmax(plan, u_add_v(plan, s, t, negative_slope)), v) and
    nothing else, so it is differentiable in s, t and v.  The heads are s.shape[1]; one-dimensional s and t are one head with (E,) weights, n x 1 one
    head with E x 1 weights as graph_attention(heads=1) has them.  With return_weights=True also the attention weights."""
    _edge_plan("gat_attention", plan)
    _edge_features("gat_attention", "v", plan, v, plan.n_cols, "n_cols")
    e = u_add_v(plan, s, t, negative_slope)
    H = int(e.shape[1]) if e.dim() == 2 else 1
    if H < 1 or int(v.shape[1]) % H != 0:
        raise _l.VglHipError("gat_attention: the width %d of v must be divisible by the heads of s and t (%d)" % (int(v.shape[1]), H))
    w = _edge_softmax_any(plan, e)
    out = spmm(plan, w, v)
    return (out, w) if return_weights else out
