"""Restatement of the k-core contract of include/vgl_hip.h (vgl_hip_kcore_run) with numpy / scipy.sparse, on tri_reference.simple_undirected.

Test support, not a test file: tests/test_kcore_cpu.py checks it on closed forms and against networkx.core_number, tests/test_kcore_gpu.py compares the
HIP path with it.
"""
import numpy as np

from tri_reference import simple_undirected


def core_numbers(V, src, dst, k_limit=0):
    """returns (core int32[V], degree int32[V], undirected_edges, distinct core values).  A synchronous peel: for the smallest remaining degree k,
    remove every vertex of degree <= k (core = k), lower its neighbours, repeat until none is left at or below k.  k_limit > 0: core =
    minimum(core, k_limit), and the last figure counts the distinct core values below k_limit (the values of k such a peel visits)."""
    A = simple_undirected(V, src, dst)
    degree = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    deg = degree.copy()
    alive = np.ones(V, dtype=bool)
    core = np.zeros(V, dtype=np.int64)
    while alive.any():
        k = int(deg[alive].min())
        front = np.flatnonzero(alive & (deg <= k))
        while front.size:
            core[front] = k
            alive[front] = False
            rows = A[front]
            touched = np.unique(rows.indices)
            deg -= np.bincount(rows.indices, minlength=V)
            touched = touched[alive[touched]]
            front = touched[deg[touched] <= k]
    distinct = np.unique(core)
    if k_limit > 0:
        distinct = distinct[distinct < k_limit]
        core = np.minimum(core, k_limit)
    return core.astype(np.int32), degree.astype(np.int32), int(A.nnz // 2), int(distinct.size)


def _clique(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


def _wheel(n):
    """hub 0, rim 1 .. n"""
    return [(0, i) for i in range(1, n + 1)] + [(i, i % n + 1) for i in range(1, n + 1)]


def _grid(n):
    at = lambda r, c: r * n + c
    return [(at(r, c), at(r, c + 1)) for r in range(n) for c in range(n - 1)] + [(at(r, c), at(r + 1, c)) for r in range(n - 1) for c in range(n)]


_TRI = [(0, 1), (1, 2), (2, 0)]
_PETERSEN = [(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)]

# closed forms: name -> (V, stored edges (src, dst), core numbers)
HAND_CASES = {
    "k5": (5, _clique(5), [4] * 5),
    "path": (6, [(i, i + 1) for i in range(5)], [1] * 6),
    "cycle": (7, [(i, (i + 1) % 7) for i in range(7)], [2] * 7),
    "star": (6, [(0, i) for i in range(1, 6)], [1] * 6),
    "tree": (7, [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (2, 6)], [1] * 7),
    "k35": (8, [(a, b) for a in range(3) for b in range(3, 8)], [3] * 8),
    "wheel_7": (8, _wheel(7), [3] * 8),
    "petersen": (10, _PETERSEN, [3] * 10),
    "grid_4x4": (16, _grid(4), [2] * 16),
    "isolated_vertices": (6, [(1, 3), (3, 4), (4, 1)], [0, 2, 0, 2, 2, 0]),
    "triangle_with_loops_and_duplicates": (3, 2 * (_TRI + [(b, a) for a, b in _TRI]) + [(0, 0), (1, 1), (2, 2)], [2] * 3),
    "k5_with_pendant_path_of_6": (11, _clique(5) + [(4, 5)] + [(i, i + 1) for i in range(5, 10)], [4] * 5 + [1] * 6),
    "k4_and_k6_joined_by_one_edge": (10, _clique(4) + _clique(6, 4) + [(3, 4)], [3] * 4 + [5] * 6),
}
