"""The personalised-PageRank contract of include/vgl_hip.h (vgl_hip_ppr_run) restated with numpy / scipy.sparse in float64: the stored entries are the
entries of a sparse count matrix (a multi-edge is an entry > 1, a self entry an edge like any other), one iteration is
    y = x / outdeg (0 on the dangling vertices),  D = sum of x over the dangling vertices,  x' = alpha A^T y + (alpha D + 1 - alpha) p,
from x = p, in batches of 16 that stop together.  Also: the dense solve the iteration converges to, the tolerance the tests use (derived in DESIGN
section 28, not measured), the supports after t iterations, and the fixed small graphs."""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
BATCH = 16


class Graph:
    """the count matrix of the stored entries and what the contract reads of it"""

    def __init__(self, V, src, dst):
        src = np.asarray(src, dtype=np.int64).ravel()
        dst = np.asarray(dst, dtype=np.int64).ravel()
        self.V = int(V)
        self.E = int(src.size)
        A = sp.coo_matrix((np.ones(src.size, dtype=np.float64), (src, dst)), shape=(V, V)).tocsr()      # duplicates are summed: multiplicities
        self.A, self.AT = A, A.T.tocsr()
        self.outdeg = np.bincount(src, minlength=V).astype(np.int64)
        self.indeg = np.bincount(dst, minlength=V).astype(np.int64)
        self.dangling = self.outdeg == 0
        self.d_max = int(self.indeg.max(initial=0))
        self.n_dangling = int(self.dangling.sum())


def teleport(V, seeds, weights=None):
    """p of one seed list: the weights over their sum, the sum added in list order; a vertex listed twice gets both; the empty list is uniform"""
    seeds = [int(s) for s in seeds]
    if not seeds:
        return np.full(V, np.float64(1.0) / np.float64(V))
    w = np.ones(len(seeds), dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    total = np.float64(0.0)
    for x in w:
        total = total + x
    p = np.zeros(V, dtype=np.float64)
    for s, x in zip(seeds, w):
        p[s] = p[s] + x / total
    return p


def step(G, x, p, alpha):
    y = np.where(G.dangling, 0.0, x / np.maximum(G.outdeg, 1).astype(np.float64))
    D = np.float64(x[G.dangling].sum())
    return np.float64(alpha) * (G.AT @ y) + (np.float64(alpha) * D + (np.float64(1.0) - np.float64(alpha))) * p


def pagerank(G, seed_lists, weights=None, alpha=0.85, max_iterations=100, tol=0.0):
    """(rank [count, V], err [count], iterations [count], stats dict) of the contract: batches of 16 in the given order, a batch stops after the first
    iteration whose largest err is <= tol (tol > 0) or at max_iterations"""
    count = len(seed_lists)
    rank = np.zeros((count, G.V), dtype=np.float64)
    err = np.zeros(count, dtype=np.float64)
    iterations = np.zeros(count, dtype=np.int32)
    st = {"sources": count, "batches": 0, "iterations_total": 0, "iterations_max": 0, "batches_converged": 0, "entries_walked": 0, "max_err": 0.0}
    for base in range(0, count, BATCH):
        members = range(base, min(base + BATCH, count))
        p = [teleport(G.V, seed_lists[j], None if weights is None else weights[j]) for j in members]
        x = [q.copy() for q in p]
        e = [0.0 for _ in members]
        t, converged = 0, False
        while t < max_iterations:
            nxt = [step(G, x[i], p[i], alpha) for i in range(len(p))]
            e = [float(np.abs(nxt[i] - x[i]).sum()) for i in range(len(p))]
            x = nxt
            t += 1
            if tol > 0 and max(e) <= tol:
                converged = True
                break
        for i, j in enumerate(members):
            rank[j], err[j], iterations[j] = x[i], e[i], t
        st["batches"] += 1
        st["iterations_total"] += t
        st["iterations_max"] = max(st["iterations_max"], t)
        st["batches_converged"] += int(converged)
        st["entries_walked"] += t * G.E
        st["max_err"] = max(st["max_err"], max(e))
    return rank, err, iterations, st


def dense_solve(G, p, alpha):
    """x* of (I - alpha (M + p dang^T)) x = (1 - alpha) p,  M[v, u] = (entries u -> v) / outdeg(u)"""
    inv = np.where(G.dangling, 0.0, 1.0 / np.maximum(G.outdeg, 1))
    M = G.AT.toarray() * inv[None, :]
    T = M + np.outer(p, G.dangling.astype(np.float64))
    return np.linalg.solve(np.eye(G.V) - alpha * T, (1.0 - alpha) * p)


def tolerance(d_max, n_dangling, alpha, t):
    """|computed - exact|_1 after t iterations: gamma_k (1 - alpha^t) / (1 - alpha), gamma_k = k u / (1 - k u), k = max(d_max, n_dangling) + 6: the
    roundings on the longest chain into one value (the sum; the division, the scaling by alpha, alpha * D, + (1 - alpha), * p and the teleport
    addition).  A test that compares two float64 evaluations uses twice it -- DESIGN section 28."""
    k = max(int(d_max), int(n_dangling)) + 6
    gamma = k * U / (1.0 - k * U)
    return gamma * (1.0 - alpha ** t) / (1.0 - alpha)


def support(G, seeds, t):
    """the vertices x_t is non-zero on, for a listed p and 0 < alpha < 1: those within t hops of the seeds along outgoing entries (the mass a
    dangling vertex hands back lands on the seeds, which are inside the set already)"""
    reach = np.zeros(G.V, dtype=bool)
    reach[[int(s) for s in seeds]] = True
    for _ in range(t):
        reach = reach | ((G.AT @ reach.astype(np.float64)) > 0)
    return reach


def _both(edges):
    return edges + [(b, a) for a, b in edges]


# name -> (V, stored entries)
SMALL = {
    "cycle_directed": (7, [(i, (i + 1) % 7) for i in range(7)]),
    "path_to_dangling": (6, [(i, i + 1) for i in range(5)]),
    "complete": (9, [(a, b) for a in range(9) for b in range(9) if a != b]),
    "star_both_ways": (8, _both([(0, i) for i in range(1, 8)])),
    "loops_and_multi_edges": (6, [(0, 1), (0, 1), (0, 1), (1, 2), (2, 2), (2, 0), (3, 3), (3, 4), (4, 0), (4, 0), (1, 1)]),
    "two_components_and_isolated": (9, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (5, 6)]),
    "all_dangling_after_one_step": (7, [(0, 4), (1, 4), (1, 5), (2, 6), (3, 5)]),
}


def small(name):
    V, edges = SMALL[name]
    src, dst = np.array([a for a, _ in edges], dtype=np.int64), np.array([b for _, b in edges], dtype=np.int64)
    return V, src, dst


def row_length_graph(lengths=(0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)):
    """vertex i has exactly lengths[i] incoming entries (sources cycle over all V vertices, so there are multi-edges and self entries only by
    accident of the cycle); the remaining vertices have none.  V = 1100 is no multiple of anything the kernels tile by."""
    V = 1100
    src, dst = [], []
    at = 0
    for v, n in enumerate(lengths):
        src.extend(((at + np.arange(n)) * 7 + 3) % V)
        dst.extend([v] * n)
        at += n
    return V, np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)
