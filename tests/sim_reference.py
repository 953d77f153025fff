"""Restatement of the vertex similarity contract of include/vgl_hip.h (vgl_hip_sim_pairs, vgl_hip_sim_topk) with numpy / scipy.sparse, and a
brute-force version over Python sets for graphs of a few hundred vertices.

Test support, not a test file: tests/test_sim_cpu.py checks it against the brute force and closed forms, tests/test_sim_gpu.py compares the HIP path
with it.  Everything here is in ONE numbering, the one its caller passes the graph in.
"""
import math
from fractions import Fraction

import numpy as np

import tri_reference as T

COMMON, JACCARD, OVERLAP = "common", "jaccard", "overlap"
METRICS = (COMMON, JACCARD, OVERLAP)


def simple_graph(V, src, dst):
    """{"V", "A": the 0/1 CSR matrix of tri_reference.simple_undirected, "deg": int64 [V], "work2": int64 [V], the 2-paths that leave every vertex}"""
    A = T.simple_undirected(V, src, dst)
    A.sort_indices()
    deg = np.asarray(A.sum(axis=1)).ravel().astype(np.int64)
    return {"V": int(V), "A": A, "deg": deg, "work2": np.asarray(A @ deg).ravel().astype(np.int64)}


def neighbours(G, u):
    A = G["A"]
    return A.indices[A.indptr[u]:A.indptr[u + 1]]


def common(G, u, v):
    """c(u_i, v_i) = (A @ A)[u_i, v_i], taken entry by entry as the row product A[u_i] . A[v_i]: int64 [n]"""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    if u.size == 0:
        return np.zeros(0, dtype=np.int64)
    return np.asarray(G["A"][u].multiply(G["A"][v]).sum(axis=1)).ravel().astype(np.int64)


def edge_common(G, block=1024):
    """(eu, ev, c): all undirected edges lo < hi in ascending (lo, hi) order (the library's edge numbering) and c = ((A @ A) o A) of each, the
    triangles through the edge; the product is taken `block` rows at a time"""
    A, V = G["A"], G["V"]
    eu, ev, c = [], [], []
    for lo in range(0, V, block):
        rows = A[lo:lo + block]
        S = (rows @ A).multiply(rows).tocsr()                        # the common neighbours of the adjacent pairs; an edge without any has no entry
        both = (rows + S).tocoo()                                    # entry = 1 + c on every edge of these rows
        up = both.col > both.row + lo
        order = np.lexsort((both.col[up], both.row[up]))
        eu.append(both.row[up][order].astype(np.int64) + lo)
        ev.append(both.col[up][order].astype(np.int64))
        c.append(both.data[up][order].astype(np.int64) - 1)
    return np.concatenate(eu), np.concatenate(ev), np.concatenate(c)


def weighted(G, u, v, weight):
    """per pair: math.fsum of weight[w] over the common neighbours w (the correctly rounded sum), and the number of hits"""
    weight = np.asarray(weight, dtype=np.float64)
    out, hits = np.zeros(len(u), dtype=np.float64), np.zeros(len(u), dtype=np.int64)
    for i, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        w = np.intersect1d(neighbours(G, a), neighbours(G, b), assume_unique=True)
        out[i] = math.fsum(weight[w].tolist())
        hits[i] = w.size
    return out, hits


def adamic_adar_weights(deg):
    d = np.asarray(deg, dtype=np.float64)
    return np.where(d >= 2, 1.0 / np.log(np.maximum(d, 2.0)), 0.0)


def resource_allocation_weights(deg):
    d = np.asarray(deg, dtype=np.float64)
    return np.where(d >= 1, 1.0 / np.maximum(d, 1.0), 0.0)


def score(metric, c, du, dv):
    """float64 score from the counts and the degrees, 0 where the denominator is 0 (what api.similarity() builds with torch)"""
    c, du, dv = (np.asarray(x, dtype=np.float64) for x in (c, du, dv))
    if metric == COMMON:
        return c
    num, den = {JACCARD: (c, du + dv - c), OVERLAP: (c, np.minimum(du, dv)), "sorensen": (2.0 * c, du + dv)}[metric]
    return np.where(den > 0, num / np.maximum(den, 1.0), 0.0)


def fraction(metric, c, du, dw):
    """(num, den) of a candidate's score as integers (arrays or scalars)"""
    if metric == COMMON:
        return c, c * 0 + 1
    if metric == JACCARD:
        return c, du + dw - c
    if metric == OVERLAP:
        return c, np.minimum(du, dw)
    if metric == "sorensen":
        return 2 * c, du + dw
    raise ValueError(metric)


def candidates(G, u, include_neighbours=False):
    """(w, c): the vertices w != u with c(u, w) >= 1, without N(u) unless include_neighbours; ascending w"""
    A = G["A"]
    row = (A[u] @ A).tocsr()
    row.sort_indices()
    w, c = row.indices.astype(np.int64), row.data.astype(np.int64)
    keep = (w != u) & (c > 0)
    if not include_neighbours:
        keep &= ~np.isin(w, neighbours(G, u))
    return w[keep], c[keep]


def ranked(G, u, metric, include_neighbours=False, label=None, k=None):
    """the candidates of u, best first under the total order (the score as an exact fraction, descending; then the smaller label): (w, c).
    k: only the first k (a float64 prefilter with a margin far above its rounding keeps every possible member of the top k and all that tie with
    them; the order among those is a Python sort under fractions.Fraction)"""
    w, c = candidates(G, u, include_neighbours)
    lab = w if label is None else np.asarray(label, dtype=np.int64)[w]
    num, den = fraction(metric, c, G["deg"][u], G["deg"][w])
    idx = np.arange(w.size)
    if k is not None and w.size > k:
        s = num / den
        kth = np.partition(s, s.size - k)[s.size - k]
        idx = np.flatnonzero(s >= kth - 1e-9 * max(1.0, abs(kth)))
    order = sorted(idx.tolist(), key=lambda i: (-Fraction(int(num[i]), int(den[i])), int(lab[i])))
    order = np.asarray(order if k is None else order[:k], dtype=np.int64)
    return w[order], c[order]


def topk(G, queries, k, metric, include_neighbours=False, label=None):
    """the restatement of vgl_hip_sim_topk: {"ids" int64 [n, k] padded with -1, "common" int64 [n, k] padded with 0, "candidates_total", "filled",
    "two_paths_walked", "queries"}"""
    queries = np.arange(G["V"]) if queries is None else np.asarray(queries, dtype=np.int64)
    ids = np.full((queries.size, k), -1, dtype=np.int64)
    com = np.zeros((queries.size, k), dtype=np.int64)
    total = filled = 0
    for i, u in enumerate(queries.tolist()):
        total += candidates(G, u, include_neighbours)[0].size
        w, c = ranked(G, u, metric, include_neighbours, label, k)
        ids[i, :w.size], com[i, :w.size] = w, c
        filled += w.size
    return {"ids": ids, "common": com, "candidates_total": int(total), "filled": int(filled), "two_paths_walked": int(G["work2"][queries].sum()),
            "queries": int(queries.size)}


def pair_stats(G, u, v, short=32, wave=1024):
    """the exact statistics of vgl_hip_sim_pairs"""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    m = np.minimum(G["deg"][u], G["deg"][v])
    return {"pairs": int(u.size), "pairs_short": int((m <= short).sum()), "pairs_wave": int(((m > short) & (m <= wave)).sum()), "pairs_wg": int((m > wave).sum()),
            "elements_examined": int(m.sum()), "common_total": int(common(G, u, v).sum())}


def pair_bytes(G, st, common_out=True, weighted_out=False, degree_out=False):
    n, V = st["pairs"], G["V"]
    return (64 * n + 4 * st["elements_examined"] + (4 * n if common_out else 0) + (8 * n + 8 * st["common_total"] + 8 * V if weighted_out else 0)
            + (8 * V if degree_out else 0))


def topk_rows(G, queries, small=1024, table=8192):
    w2 = G["work2"][np.arange(G["V"]) if queries is None else np.asarray(queries, dtype=np.int64)]
    return {"rows_small": int((w2 <= small).sum()), "rows_table": int(((w2 > small) & (w2 <= table)).sum()), "rows_global": int((w2 > table).sum())}


def topk_bytes(ref, k, common_out=True):
    return 36 * ref["queries"] + 4 * ref["two_paths_walked"] + (8 if common_out else 4) * ref["queries"] * k


# ---- brute force over Python sets, for graphs of a few hundred vertices ----
def brute_sets(V, stored):
    N = [set() for _ in range(V)]
    for a, b in stored:
        if a != b:
            N[a].add(b)
            N[b].add(a)
    return N


def brute_common(N, pairs):
    return [len(N[a] & N[b]) for a, b in pairs]


def brute_topk(N, u, k, metric, include_neighbours=False, label=None):
    """[(w, c)]: best first, at most k"""
    out = []
    for w in range(len(N)):
        c = len(N[u] & N[w])
        if w == u or c == 0 or (not include_neighbours and w in N[u]):
            continue
        du, dw = len(N[u]), len(N[w])
        s = {COMMON: Fraction(c), JACCARD: Fraction(c, du + dw - c), OVERLAP: Fraction(c, min(du, dw)), "sorensen": Fraction(2 * c, du + dw)}[metric]
        out.append((-s, w if label is None else int(label[w]), w, c))
    out.sort()
    return [(w, c) for _, _, w, c in out[:k]]


def _clique(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


# hand cases: name -> (V, stored entries)
HAND_CASES = {
    "k6": (6, _clique(6)),
    "k34": (7, [(a, b) for a in range(3) for b in range(3, 7)]),
    "path5": (5, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    "star": (8, [(0, i) for i in range(1, 7)]),                        # hub 0, leaves 1 .. 6, vertex 7 isolated
    "two_triangles_sharing_a_vertex": (5, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 2)]),
    "edgeless": (4, []),
    "loops_and_duplicates": (5, [(0, 0), (0, 1), (1, 0), (0, 1), (1, 2), (2, 1), (2, 2), (0, 2), (2, 3), (3, 2), (3, 3), (3, 4)]),
}


def hand_graph(name):
    V, stored = HAND_CASES[name]
    src = np.asarray([a for a, _ in stored], dtype=np.int64)
    dst = np.asarray([b for _, b in stored], dtype=np.int64)
    return V, src, dst, simple_graph(V, src, dst)
