"""Restatement of the triangle counting contract of include/vgl_hip.h (vgl_hip_tri_run) with numpy / scipy.sparse.

Test support, not a test file: tests/test_tri_cpu.py checks it on hand-made cases and against dense A^3, tests/test_tri_gpu.py compares the HIP path
with it.  (`tc` in this tree is transitive closure; triangle counting is `tri`.)
"""
import numpy as np
import scipy.sparse as sp


def simple_undirected(V, src, dst):
    """the simple undirected graph underlying the stored entries: symmetrise, drop the diagonal, deduplicate -> 0/1 CSR matrix (int64)"""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    keep = src != dst
    s, d = src[keep], dst[keep]
    A = sp.coo_matrix((np.ones(2 * s.size, dtype=np.int64), (np.concatenate([s, d]), np.concatenate([d, s]))), shape=(V, V)).tocsr()
    A.sum_duplicates()
    A.data[:] = 1
    return A


def triangle_count(V, src, dst, rank=None):
    """returns (triangles, per_vertex int64[V], degree int32[V], undirected_edges).  rank: any total order (a permutation of 0..V-1, the position of
    each vertex); default (degree, id).  The answer does not depend on it."""
    A = simple_undirected(V, src, dst)
    deg = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    if rank is None:
        rank = np.empty(V, dtype=np.int64)
        rank[np.lexsort((np.arange(V), deg))] = np.arange(V)
    rank = np.asarray(rank, dtype=np.int64)
    C = A.tocoo()
    up = rank[C.row] < rank[C.col]
    L = sp.csr_matrix((np.ones(int(up.sum()), dtype=np.int64), (C.row[up], C.col[up])), shape=(V, V))     # every edge once, lower -> higher
    B = (L @ L).multiply(L).tocsr()              # B[a, b] = triangles a < c < b of the oriented edge (a, b): every triangle once
    M = (L.T @ L).multiply(L).tocsr()            # M[c, b] = triangles a < c < b of the oriented edge (c, b)
    T = int(B.sum())
    low = np.asarray(B.sum(axis=1)).ravel()
    high = np.asarray(B.sum(axis=0)).ravel()
    mid = np.asarray(M.sum(axis=1)).ravel()
    per_vertex = (low + high + mid).astype(np.int64)
    return T, per_vertex, deg.astype(np.int32), int(L.nnz)


def clustering(per_vertex, degree):
    """local clustering coefficient 2 t / (d (d - 1)) in float64, 0 where d < 2"""
    d = np.asarray(degree).astype(np.float64)
    pairs = d * (d - 1.0)
    return np.where(np.asarray(degree) >= 2, 2.0 * np.asarray(per_vertex).astype(np.float64) / np.maximum(pairs, 1.0), 0.0)


def brute_force(V, src, dst):
    """dense A^3: (trace / 6, diag / 2, degree) -- for graphs of a few hundred vertices"""
    A = np.zeros((V, V), dtype=np.int64)
    A[np.asarray(src), np.asarray(dst)] = 1
    A = ((A + A.T) > 0).astype(np.int64)
    np.fill_diagonal(A, 0)
    A3 = A @ A @ A
    return int(np.trace(A3) // 6), (np.diag(A3) // 2).astype(np.int64), A.sum(axis=1).astype(np.int32)


def _clique(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def _wheel(n):
    """hub 0, rim 1 .. n"""
    return [(0, i) for i in range(1, n + 1)] + [(i, i % n + 1) for i in range(1, n + 1)]


_TRI = [(0, 1), (1, 2), (2, 0)]

# hand-checked cases: name -> (V, stored edges (src, dst), triangles, per-vertex counts)
HAND_CASES = {
    "triangle": (3, [(0, 1), (1, 2), (0, 2)], 1, [1, 1, 1]),
    "k4": (4, _clique(4), 4, [3] * 4),
    "k5": (5, _clique(5), 10, [6] * 5),
    "path": (5, [(0, 1), (1, 2), (2, 3), (3, 4)], 0, [0] * 5),
    "star": (5, [(0, 1), (0, 2), (0, 3), (0, 4)], 0, [0] * 5),
    "even_cycle": (6, [(i, (i + 1) % 6) for i in range(6)], 0, [0] * 6),
    "k33": (6, [(a, b) for a in range(3) for b in range(3, 6)], 0, [0] * 6),
    "two_triangles_sharing_an_edge": (4, [(0, 1), (1, 2), (0, 2), (1, 3), (2, 3)], 2, [1, 2, 2, 1]),
    "directed_3_cycle_one_way": (3, _TRI, 1, [1, 1, 1]),
    "3_cycle_both_ways_twice": (3, 2 * (_TRI + [(b, a) for a, b in _TRI]), 1, [1, 1, 1]),
    "self_loops_on_a_triangle": (3, _TRI + [(0, 0), (1, 1), (2, 2)], 1, [1, 1, 1]),
    "isolated_vertices": (6, [(1, 3), (3, 4), (4, 1)], 1, [0, 1, 0, 1, 1, 0]),
    "wheel_4": (5, _wheel(4), 4, [4, 2, 2, 2, 2]),
    "wheel_7": (8, _wheel(7), 7, [7] + [2] * 7),
}
