"""Restatement of the k-truss contract of include/vgl_hip.h (vgl_hip_ktruss_run) with numpy / scipy.sparse, on tri_reference.simple_undirected.

Test support, not a test file: tests/test_ktruss_cpu.py checks it on closed forms and against networkx.k_truss, tests/test_ktruss_gpu.py compares the
HIP path with it.
"""
import numpy as np
import scipy.sparse as sp

from tri_reference import simple_undirected


def edge_list(V, src, dst):
    """the simple undirected graph and its edges {lo < hi} in ascending (lo, hi) order: (A, edge_u int32[E'], edge_v int32[E'])"""
    A = simple_undirected(V, src, dst)
    U = sp.triu(A, k=1).tocsr()
    U.sort_indices()
    lo = np.repeat(np.arange(V, dtype=np.int64), np.diff(U.indptr))
    return A, lo.astype(np.int32), U.indices.astype(np.int32)


def truss_numbers(V, src, dst, k_limit=0):
    """returns (edge_u int32[E'], edge_v int32[E'], truss int32[E'], support int32[E'], triangles, rounds, sub_rounds).  A synchronous peel: for
    k = the smallest support of an alive edge + 2, remove every alive edge of support <= k - 2 (truss = k), lower the supports of the remaining edges
    by the triangles that went with the removed ones, repeat until none is left at or below k - 2.  rounds counts the values of k, sub_rounds the
    removals.  k_limit >= 2: the peel stops when k reaches it and every remaining edge gets k_limit.
    Incremental: with R the remaining edges and F the removed ones, the triangles an edge of R loses are ((F R) + (F R)^T + F F) o R."""
    if k_limit < 0 or k_limit == 1:
        raise ValueError("k_limit must be 0 or at least 2")
    A, eu, ev = edge_list(V, src, dst)
    E = int(eu.size)
    keys = eu.astype(np.int64) * V + ev                              # ascending: the edge numbering
    A = A.tocsr()
    A.sort_indices()
    rows = np.repeat(np.arange(V, dtype=np.int64), np.diff(A.indptr))
    slot_eid = np.searchsorted(keys, np.minimum(rows, A.indices) * V + np.maximum(rows, A.indices))      # the edge of every adjacency slot
    S = (A @ A).multiply(A).tocsr()
    support = np.zeros(E, dtype=np.int64)
    c = sp.triu(S, k=1).tocoo()
    support[np.searchsorted(keys, c.row.astype(np.int64) * V + c.col)] = c.data
    triangles = int(support.sum()) // 3
    sup = support.copy()
    alive = np.ones(E, dtype=bool)
    truss = np.zeros(E, dtype=np.int64)
    rounds = sub_rounds = 0
    while alive.any():
        k = int(sup[alive].min()) + 2
        if k_limit and k >= k_limit:
            truss[alive] = k_limit
            break
        rounds += 1
        front = np.flatnonzero(alive & (sup <= k - 2))
        while front.size:
            sub_rounds += 1
            truss[front] = k
            alive[front] = False
            keep = alive[slot_eid]                                    # the remaining graph (own arrays: A is left as it is)
            R = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int64), (rows[keep], A.indices[keep])), shape=(V, V))
            fu, fv = eu[front].astype(np.int64), ev[front].astype(np.int64)
            F = sp.csr_matrix((np.ones(2 * front.size, dtype=np.int64), (np.concatenate([fu, fv]), np.concatenate([fv, fu]))), shape=(V, V))
            X = F @ R
            D = sp.triu((X + X.T + F @ F).multiply(R), k=1).tocoo()
            hit = np.searchsorted(keys, D.row.astype(np.int64) * V + D.col)
            sup[hit] -= D.data
            touched = hit[D.data > 0]
            front = touched[sup[touched] <= k - 2]
    return eu, ev, truss.astype(np.int32), support.astype(np.int32), triangles, rounds, sub_rounds


def _clique(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


def _wheel(n):
    """hub 0, rim 1 .. n"""
    return [(0, i) for i in range(1, n + 1)] + [(i, i % n + 1) for i in range(1, n + 1)]


def _case(V, stored, truss_of):
    """(V, stored edges, expected truss per edge in ascending (lo, hi) order); truss_of: one value for all, or a function of (lo, hi)"""
    simple = sorted({(min(a, b), max(a, b)) for a, b in stored if a != b})
    return V, stored, [truss_of(lo, hi) if callable(truss_of) else truss_of for lo, hi in simple]


_TRI = [(0, 1), (1, 2), (2, 0)]
_OCTAHEDRON = [(a, b) for a in range(6) for b in range(a + 1, 6) if b != a + 3]      # K_{2,2,2}: everything but the three antipodal pairs

# closed forms: name -> (V, stored edges (src, dst), truss numbers in ascending (lo, hi) order)
HAND_CASES = {
    "triangle": _case(3, [(0, 1), (1, 2), (0, 2)], 3),
    "k4": _case(4, _clique(4), 4),
    "k5": _case(5, _clique(5), 5),
    "k7": _case(7, _clique(7), 7),
    "path": _case(5, [(i, i + 1) for i in range(4)], 2),
    "star": _case(6, [(0, i) for i in range(1, 6)], 2),
    "k33": _case(6, [(a, b) for a in range(3) for b in range(3, 6)], 2),
    "diamond": _case(4, [(0, 1), (1, 2), (0, 2), (1, 3), (2, 3)], 3),
    "octahedron": _case(6, _OCTAHEDRON, 4),
    "wheel_7": _case(8, _wheel(7), 3),
    "k4_and_k6_joined_by_one_edge": _case(10, _clique(4) + _clique(6, 4) + [(3, 4)], lambda lo, hi: 4 if hi <= 3 else 6 if lo >= 4 else 2),
    # a double decrement of the shared edge (0, 1) would take the K4 down to 3
    "k4_with_pendant_triangle_on_an_edge": _case(5, _clique(4) + [(0, 4), (1, 4)], lambda lo, hi: 3 if hi == 4 else 4),
    "triangle_with_loops_and_duplicates": _case(3, 2 * (_TRI + [(b, a) for a, b in _TRI]) + [(0, 0), (1, 1), (2, 2)], 3),
    "isolated_vertices": _case(7, [(1, 3), (3, 4), (4, 1), (4, 6)], lambda lo, hi: 2 if hi == 6 else 3),
    "empty": _case(4, [], 2),
    "only_loops": _case(4, [(0, 0), (2, 2), (2, 2)], 2),
}


def tube(n, capped_both=False):
    """(V, src, dst): n rings of 4 vertices (ring j: 4j .. 4j + 3, a 4-cycle), ring j joined to ring j + 1 by (4j + i, 4j + 4 + i) and
    (4j + i, 4j + 4 + (i + 1) % 4), an apex over ring 0 and, capped_both, one over ring n - 1.  Capped at both ends every edge is in exactly two
    triangles (truss 4, one sub-round); with one end open the peel walks the tube from that end, a ring at a time (truss 3)."""
    e = []
    for j in range(n):
        for i in range(4):
            e.append((4 * j + i, 4 * j + (i + 1) % 4))
            if j + 1 < n:
                e.append((4 * j + i, 4 * j + 4 + i))
                e.append((4 * j + i, 4 * j + 4 + (i + 1) % 4))
    V = 4 * n + 1
    e += [(4 * n, i) for i in range(4)]
    if capped_both:
        e += [(4 * n + 1, 4 * (n - 1) + i) for i in range(4)]
        V += 1
    s, d = zip(*e)
    return V, np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)


def book(n):
    """(V, src, dst): the spine (0, 1) and n pages w ~ 0, w ~ 1: n triangles that share the spine"""
    w = np.arange(2, n + 2, dtype=np.int64)
    return n + 2, np.concatenate([[0], np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)]), np.concatenate([[1], w, w])


def tripartite(m):
    """(V, src, dst): the complete tripartite graph K_{m,m,m} (truss m + 2)"""
    a = np.arange(m, dtype=np.int64)
    s, d = np.repeat(a, m), np.tile(a, m)
    return 3 * m, np.concatenate([s, s, s + m]), np.concatenate([d + m, d + 2 * m, d + 2 * m])
