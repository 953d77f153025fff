"""The betweenness-centrality contract of include/vgl_hip.h (vgl_hip_bc_run) restated with numpy / scipy.sparse, level-synchronously: the stored
entries are the entries of a sparse count matrix A (a multi-edge is an entry > 1), sigma of level l + 1 is A^T (sigma masked to level l) on the vertices
not seen before, delta of level l is sigma * (A (coef masked to level l + 1)) with coef = (1 + delta) / sigma.  Levels are written as vgl_hip_bfs_run
writes them: source 1, unreached -1.  Also: the tolerance the tests use (derived in DESIGN section 14, not measured), a brute force that shares nothing
with the restatement but the definition (all-pairs distance and path-count matrices), the certificate that needs no reference, and the hand cases."""
import math

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53


def count_matrix(V, src, dst):
    src = np.asarray(src, dtype=np.int64).ravel()
    dst = np.asarray(dst, dtype=np.int64).ravel()
    A = sp.coo_matrix((np.ones(src.size, dtype=np.float64), (src, dst)), shape=(V, V)).tocsr()      # duplicates are summed: multiplicities
    return A, A.T.tocsr()


def single_source(A, AT, s):
    """(levels int32, sigma f64, delta f64, D) of one source"""
    V = A.shape[0]
    levels = np.full(V, -1, dtype=np.int32)
    sigma = np.zeros(V, dtype=np.float64)
    levels[s], sigma[s] = 1, 1.0
    cur = 1
    while True:
        reach = AT @ np.where(levels == cur, sigma, 0.0)
        new = (reach > 0) & (levels == -1)
        if not new.any():
            break
        levels[new] = cur + 1
        sigma[new] = reach[new]
        cur += 1
    D = cur - 1
    delta = np.zeros(V, dtype=np.float64)
    coef = np.zeros(V, dtype=np.float64)
    for l in range(D + 1, 0, -1):
        here = levels == l
        if l <= D:
            t = A @ np.where(levels == l + 1, coef, 0.0)
            delta[here] = sigma[here] * t[here]
        coef[here] = (1.0 + delta[here]) / sigma[here]
    return levels, sigma, delta, D


def betweenness(V, src, dst, sources=None):
    """bc (f64, directed, unnormalised, endpoints not counted) and the integers vgl_hip_bc_stats reports, plus what the tolerance needs"""
    A, AT = count_matrix(V, src, dst)
    outdeg = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    indeg = np.asarray(AT.sum(axis=1)).ravel().astype(np.int64)
    sources = list(range(V)) if sources is None else [int(s) for s in sources]
    bc = np.zeros(V, dtype=np.float64)
    info = {"sources": len(sources), "max_depth": 0, "levels_total": 0, "reached_total": 0, "edges_forward": 0, "edges_backward": 0, "sigma_max": 0.0,
            "d_max": int(max(outdeg.max(initial=0), indeg.max(initial=0))), "certificate": []}
    for s in sources:
        levels, sigma, delta, D = single_source(A, AT, s)
        reached = levels > 0
        add = delta.copy()
        add[s] = 0.0
        bc += add
        info["max_depth"] = max(info["max_depth"], D)
        info["levels_total"] += D + 1
        info["reached_total"] += int(reached.sum())
        info["edges_forward"] += int(indeg[levels > 1].sum())
        info["edges_backward"] += int(outdeg[reached & (levels <= D)].sum())
        info["sigma_max"] = max(info["sigma_max"], float(sigma.max(initial=0.0)))
        info["certificate"].append(certificate(levels))
        info["last"] = (levels, sigma, delta)
    return bc, info


def certificate(levels):
    """sum over v != s of delta_s[v] = sum over the reached t != s of (d(s, t) - 1): every pair contributes the interior vertices of its shortest
    paths, averaged (delta_s[s] itself is the number of reached t != s and is not part of bc).  An integer from the levels alone."""
    levels = np.asarray(levels, dtype=np.int64)
    return int((levels[levels > 1] - 2).sum())


def tolerance(D, d_max, S):
    """relative, per vertex: 2 (D (d_max + 4) + S) 2^-53 -- DESIGN section 14"""
    return 2.0 * (D * (d_max + 4) + S) * U


def compare(got, ref, tol):
    """(ok, largest |got - ref| / (tol * ref)): within tol relative where ref != 0, exactly 0 where ref == 0"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    zero = ref == 0
    ok = bool(np.all(got[zero] == 0))
    frac = 0.0
    if (~zero).any():
        frac = float(np.max(np.abs(got[~zero] - ref[~zero]) / (tol * ref[~zero])))
    return ok and frac <= 1.0, frac


def brute_force(V, src, dst):
    """all sources, from all-pairs matrices: dist[s, t] = the first k with (A^k)[s, t] > 0, paths[s, t] = that entry (walks of the shortest length are
    the shortest paths); bc[v] = sum over s != v != t with d(s, v) + d(v, t) = d(s, t) of paths[s, v] paths[v, t] / paths[s, t]"""
    M = np.zeros((V, V), dtype=np.float64)
    np.add.at(M, (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)), 1.0)
    dist = np.full((V, V), -1, dtype=np.int64)
    paths = np.zeros((V, V), dtype=np.float64)
    np.fill_diagonal(dist, 0)
    np.fill_diagonal(paths, 1.0)
    P = np.eye(V)
    for k in range(1, V):
        P = P @ M
        new = (P > 0) & (dist < 0)
        if not new.any():
            break
        dist[new] = k
        paths[new] = P[new]
    bc = np.zeros(V, dtype=np.float64)
    for v in range(V):
        dsv, dvt = dist[:, v][:, None], dist[v, :][None, :]
        on = (dsv > 0) & (dvt > 0) & (dist > 0) & (dsv + dvt == dist)
        num = paths[:, v][:, None] * paths[v, :][None, :]
        bc[v] = float(np.sum(np.where(on, num / np.where(on, paths, 1.0), 0.0)))
    return bc


def _both(edges):
    return edges + [(b, a) for a, b in edges]


_PATH6 = [(i, i + 1) for i in range(5)]
_CYCLE6 = [(i, (i + 1) % 6) for i in range(6)]
_DIAMOND = [(0, 1), (0, 2), (1, 3), (2, 3)]
# name -> (V, stored entries, bc of all sources)
HAND_CASES = {
    "path_directed": (6, _PATH6, [float(i * (5 - i)) for i in range(6)]),
    "path_both_ways": (6, _both(_PATH6), [2.0 * i * (5 - i) for i in range(6)]),
    "star_both_ways": (6, _both([(0, i) for i in range(1, 6)]), [20.0, 0.0, 0.0, 0.0, 0.0, 0.0]),
    "cycle_directed": (5, [(i, (i + 1) % 5) for i in range(5)], [6.0] * 5),
    "cycle_both_ways": (6, _both(_CYCLE6), [4.0] * 6),
    "diamond": (4, _DIAMOND, [0.0, 0.5, 0.5, 0.0]),
    "diamond_double_edge": (4, [(0, 1)] + _DIAMOND, [0.0, 2.0 / 3.0, 1.0 / 3.0, 0.0]),
    "diamond_with_self_loops": (4, _DIAMOND + [(0, 0), (1, 1), (3, 3), (1, 1)], [0.0, 0.5, 0.5, 0.0]),
    "path_both_ways_with_self_loop": (6, _both(_PATH6) + [(2, 2)], [2.0 * i * (5 - i) for i in range(6)]),
    "two_components": (7, [(0, 1), (1, 2), (3, 4), (4, 5), (5, 6)], [0.0, 1.0, 0.0, 0.0, 2.0, 2.0, 0.0]),
    "source_without_out_edges": (4, [(0, 1), (1, 2)], [0.0, 1.0, 0.0, 0.0]),
}


def grid_both_ways(n):
    """n x n grid, vertex r * n + c, every edge stored both ways; from the corner 0 sigma[(r, c)] = C(r + c, r)"""
    idx = np.arange(n * n, dtype=np.int64).reshape(n, n)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return np.concatenate([a, b]), np.concatenate([b, a])


def grid_sigma(n):
    return np.array([[float(math.comb(r + c, r)) for c in range(n)] for r in range(n)]).ravel()
