"""Restatement of the minimum spanning forest contract of include/vgl_hip.h (vgl_hip_msf_run) with numpy / scipy.sparse, on
tri_reference.simple_undirected and ktruss_reference.edge_list (the library's edge numbering: ascending (lo, hi)).

Test support, not a test file: tests/test_msf_cpu.py checks it on hand-made cases and against networkx / scipy, tests/test_msf_gpu.py compares the HIP
path with it.
"""
import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from ktruss_reference import edge_list

INF = float("inf")


def folded(V, src, dst, w):
    """(edge_u int32[E'], edge_v int32[E'], edge_w float32[E']): the undirected edges in the library's numbering, each with the smallest weight over
    its stored copies in either direction (-0.0 counts as +0.0).  Loops are ignored, weights included; a NaN on another entry is an error."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    w = np.asarray(w, dtype=np.float32)
    assert src.size == dst.size == w.size
    _, eu, ev = edge_list(V, src, dst)
    keep = src != dst
    s, d, x = src[keep], dst[keep], w[keep] + np.float32(0.0)       # -0.0 + 0.0 = +0.0
    if np.isnan(x).any():
        raise ValueError("weights holds a NaN on an entry that is not a loop")
    keys = eu.astype(np.int64) * V + ev
    at = np.searchsorted(keys, np.minimum(s, d) * V + np.maximum(s, d))
    ew = np.full(eu.size, np.inf, dtype=np.float32)
    np.minimum.at(ew, at, x)
    return eu, ev, ew


def edge_order(ew):
    """the edge ids in ascending (weight, id): the strict total order of the contract"""
    return np.lexsort((np.arange(ew.size), ew))


def kruskal(V, eu, ev, ew):
    """bool[E']: the forest.  The edges in ascending (weight, id); an edge joins iff its ends lie in different trees."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    forest = np.zeros(eu.size, dtype=bool)
    lo, hi = eu.tolist(), ev.tolist()
    for e in edge_order(ew).tolist():
        a, b = find(lo[e]), find(hi[e])
        if a != b:
            parent[max(a, b)] = min(a, b)
            forest[e] = True
    return forest


def _labels(V, eu, ev, mask):
    """component label of every vertex of the graph with the edges `mask`"""
    G = sp.csr_matrix((np.ones(int(mask.sum()), dtype=np.int8), (eu[mask], ev[mask])), shape=(V, V))
    return connected_components(G, directed=False)[1]


def boruvka(V, eu, ev, ew):
    """(forest bool[E'], rounds): synchronous Boruvka.  In a round every component that has a crossing edge picks its smallest crossing edge under
    (weight, id); all picked edges join the forest; the components are merged along all of them before the next round.  rounds counts the rounds that
    added an edge."""
    E = int(eu.size)
    rank = np.empty(E, dtype=np.int64)
    order = edge_order(ew)
    rank[order] = np.arange(E)
    forest = np.zeros(E, dtype=bool)
    comp = np.arange(V)
    rounds = 0
    while True:
        cu, cv = comp[eu], comp[ev]
        cross = cu != cv
        if not cross.any():
            break
        best = np.full(V, E, dtype=np.int64)
        np.minimum.at(best, cu[cross], rank[cross])
        np.minimum.at(best, cv[cross], rank[cross])
        picked = order[np.unique(best[best < E])]
        assert not forest[picked].any()
        forest[picked] = True
        rounds += 1
        comp = _labels(V, eu, ev, forest)
    return forest, rounds


def components(V, eu, ev, forest):
    """int32[V]: the smallest vertex id of the vertex's tree of the forest (an isolated vertex is its own)"""
    lab = _labels(V, eu, ev, forest)
    smallest = np.full(V, V, dtype=np.int64)
    np.minimum.at(smallest, lab, np.arange(V))
    return smallest[lab].astype(np.int32)


def minimum_spanning_forest(V, src, dst, w):
    """dict: edge_u, edge_v, edge_w (all E' edges), forest (bool[E']), component (int32[V]), rounds, forest_edges, components, undirected_edges,
    total (math.fsum of the forest weights as float64).  The Boruvka restatement must give Kruskal's forest."""
    eu, ev, ew = folded(V, src, dst, w)
    forest = kruskal(V, eu, ev, ew)
    again, rounds = boruvka(V, eu, ev, ew)
    assert np.array_equal(forest, again), "synchronous Boruvka and Kruskal disagree: the order (weight, id) is not strict somewhere"
    n = int(forest.sum())
    return {"edge_u": eu, "edge_v": ev, "edge_w": ew, "forest": forest, "component": components(V, eu, ev, forest), "rounds": rounds, "forest_edges": n,
            "components": V - n, "undirected_edges": int(eu.size), "total": math.fsum(ew[forest].astype(np.float64).tolist())}


def _ring(n):
    return [(i, (i + 1) % n) for i in range(n)]


def _clique(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


# hand-checked cases: name -> (V, stored entries (src, dst, weight), the forest as sorted (lo, hi) pairs)
HAND_CASES = {
    "empty": (4, [], []),
    "only_loops": (4, [(0, 0, 1.0), (2, 2, -5.0), (2, 2, 0.5)], []),
    "isolated_vertices": (7, [(1, 3, 2.0), (3, 4, 1.0), (4, 1, 3.0), (4, 6, 5.0)], [(1, 3), (3, 4), (4, 6)]),
    "single_edge": (2, [(1, 0, -3.5)], [(0, 1)]),
    # all weights equal: without the tie-break by edge id every vertex picks "its" edge and the picks close the cycle
    "triangle_all_equal": (3, [(a, b, 1.0) for a, b in [(0, 1), (1, 2), (2, 0)]], [(0, 1), (0, 2)]),
    "ring_5_all_equal": (5, [(a, b, 1.0) for a, b in _ring(5)], [(0, 1), (0, 4), (1, 2), (2, 3)]),
    # the ring stored both ways with another weight per direction, plus duplicates: the lightest copy counts -> 1, 2, 3, 4 and 5 on (0, 4)
    "ring_5_both_ways_and_duplicates": (5, [(0, 1, 9.0), (1, 0, 1.0), (1, 2, 2.0), (2, 1, 7.0), (2, 3, 8.0), (3, 2, 6.0), (2, 3, 3.0), (3, 4, 4.0), (4, 3, 4.0),
                                            (4, 0, 5.0), (0, 4, 10.0), (0, 4, 5.5), (3, 3, -1.0)], [(0, 1), (1, 2), (2, 3), (3, 4)]),
    "k4_distinct": (4, [(0, 1, 1.0), (0, 2, 4.0), (0, 3, 3.0), (1, 2, 2.0), (1, 3, 6.0), (2, 3, 5.0)], [(0, 1), (0, 3), (1, 2)]),
    "two_components": (6, [(0, 1, 1.0), (1, 2, 2.0), (0, 2, 3.0), (3, 4, 1.0), (4, 5, 1.0), (3, 5, 1.0)], [(0, 1), (1, 2), (3, 4), (3, 5)]),
    # -0.0 equals +0.0: the tie goes to the edge ids; ordered by their bit patterns (1, 2) would come first and push (0, 2) out
    "signed_zeros": (3, [(0, 1, 0.0), (0, 2, 0.0), (1, 2, -0.0)], [(0, 1), (0, 2)]),
    "inf_bridge": (5, [(0, 1, 1.0), (1, 2, INF), (2, 3, 2.0), (3, 4, 3.0), (2, 4, INF)], [(0, 1), (1, 2), (2, 3), (3, 4)]),
    "minus_inf_edge": (3, [(0, 1, -INF), (1, 2, 1.0), (0, 2, -5.0)], [(0, 1), (0, 2)]),
}


def hand_case(name):
    """(V, src, dst, w float32, forest pairs) of a hand case"""
    V, stored, want = HAND_CASES[name]
    return (V, np.asarray([a for a, _, _ in stored], dtype=np.int64), np.asarray([b for _, b, _ in stored], dtype=np.int64),
            np.asarray([x for _, _, x in stored], dtype=np.float32), want)


def star(n):
    """(V, src, dst, w): hub 0 and n leaves, all weights equal: every leaf picks its edge, one round"""
    leaves = np.arange(1, n + 1, dtype=np.int64)
    return n + 1, np.zeros(n, dtype=np.int64), leaves, np.ones(n, dtype=np.float32)


def ruler(path=4096, clique=600):
    """(V, src, dst, w): the path 0 - 1 - ... - `path`, edge i between i and i + 1 of weight 2 + the number of trailing zero bits of i + 1, hanging off
    vertex `path` of a clique (vertices path .. path + clique - 1) whose edges all weigh 1.  The path merges pairwise, a level of the ruler per round;
    the clique is one component after the first round and its rows have no crossing entry from then on."""
    i = np.arange(path, dtype=np.int64)
    tz = np.zeros(path, dtype=np.int64)
    x = i + 1
    for _ in range(64):
        even = (x & 1) == 0
        if not even.any():
            break
        tz += even
        x = np.where(even, x >> 1, x)
    ks, kd = zip(*_clique(clique, path))
    return (path + clique, np.concatenate([i, np.asarray(ks, dtype=np.int64)]), np.concatenate([i + 1, np.asarray(kd, dtype=np.int64)]),
            np.concatenate([2.0 + tz, np.ones(len(ks))]).astype(np.float32))
