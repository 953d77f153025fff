"""numpy / scipy restatement of the multi-source BFS contract (include/vgl_hip.h, vgl_hip_msbfs_run): level by level, a sparse 0/1 matrix times a
V x k indicator block per batch of 64 sources.  Everything is integer and exact except harmonic, which is the contract's loop in float64:
h = 0; for d = 1 .. ecc ascending: h = h + n_d / d."""
import numpy as np
import scipy.sparse as sp

BATCH = 64


def step_matrix(V, src, dst, direction="out"):
    """M with M[w, v] > 0 iff the traversal goes from v to w in one step: a stored entry (v, w) for "out", (w, v) for "in"; and the
    traversal-direction degree of every vertex (stored entries, multiplicities and loops included: what a push level walks)"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    frm, to = (src, dst) if direction == "out" else (dst, src)
    M = sp.csr_matrix((np.ones(frm.size, dtype=np.int32), (to, frm)), shape=(V, V))
    M.data[:] = 1                                  # (duplicates were summed: multi-edges have no effect on distances)
    return M, np.bincount(frm, minlength=V).astype(np.int64)


def multi_source_bfs(V, src, dst, sources, direction="out", want_levels=True):
    """dict: reached, dist_sum (int64), ecc (int32), harmonic (float64) per source in source order; levels [len(sources), V] int32 (source 1,
    unreached -1) when want_levels; and the stats of an ALL-PUSH schedule: batches, max_depth, levels_total, reached_total, edges_push"""
    sources = np.asarray(list(sources), dtype=np.int64)
    n = sources.size
    assert n == 0 or (sources.min() >= 0 and sources.max() < V)
    M, deg = step_matrix(V, src, dst, direction)
    out = {"reached": np.ones(n, dtype=np.int64), "dist_sum": np.zeros(n, dtype=np.int64), "ecc": np.zeros(n, dtype=np.int32),
           "harmonic": np.zeros(n, dtype=np.float64), "batches": 0, "max_depth": 0, "levels_total": 0, "reached_total": 0, "edges_push": 0}
    levels = np.full((n, V), -1, dtype=np.int32) if want_levels else None
    for base in range(0, n, BATCH):
        s = sources[base:base + BATCH]
        k = s.size
        cols = np.arange(k)
        F = np.zeros((V, k), dtype=np.int32)
        F[s, cols] = 1
        seen = F.astype(bool)
        if want_levels:
            levels[base + cols, s] = 1
        h = np.zeros(k, dtype=np.float64)
        d = 0
        while True:
            in_frontier = F.any(axis=1)                # a vertex whose frontier word is non-zero, once whatever the number of bits
            if not in_frontier.any():
                break
            out["levels_total"] += 1
            out["edges_push"] += int(deg[in_frontier].sum())
            d += 1
            N = (np.asarray(M @ F) > 0) & ~seen
            n_d = N.sum(axis=0).astype(np.int64)
            hit = n_d > 0
            seen |= N
            out["reached"][base:base + k] += n_d
            out["dist_sum"][base:base + k] += n_d * d
            out["ecc"][base:base + k][hit] = d
            h = np.where(hit, h + n_d.astype(np.float64) / np.float64(d), h)
            if want_levels:
                vs, bs = np.nonzero(N)
                levels[base + bs, vs] = d + 1
            F = N.astype(np.int32)
        out["harmonic"][base:base + k] = h
        out["batches"] += 1
    out["max_depth"] = int(out["ecc"].max()) if n else 0
    out["reached_total"] = int(out["reached"].sum())
    if want_levels:
        out["levels"] = levels
    return out


def closeness(res, V, wf_improved=True):
    """float64 (r - 1) / dist_sum, times (r - 1) / (V - 1) when wf_improved, 0 where dist_sum == 0"""
    r1 = (res["reached"] - 1).astype(np.float64)
    tot = res["dist_sum"].astype(np.float64)
    c = np.where(tot > 0, r1 / np.maximum(tot, 1.0), 0.0)
    return c * (r1 / float(V - 1)) if (wf_improved and V > 1) else c


def queue_bfs(V, src, dst, source, direction="out"):
    """independent of the above: a plain queue over adjacency lists; distances, -1 where unreached"""
    frm, to = (src, dst) if direction == "out" else (dst, src)
    order = np.argsort(np.asarray(frm), kind="stable")
    adj = np.asarray(to)[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(frm), minlength=V))])
    dist = np.full(V, -1, dtype=np.int64)
    dist[source] = 0
    queue, head = [int(source)], 0
    while head < len(queue):
        u = queue[head]
        head += 1
        for w in adj[ptr[u]:ptr[u + 1]].tolist():
            if dist[w] < 0:
                dist[w] = dist[u] + 1
                queue.append(w)
    return dist


def sums_of(dist):
    """(reached, dist_sum, ecc, harmonic by the contract's loop) of one distance array"""
    d = dist[dist >= 0]
    ecc = int(d.max())
    n_d = np.bincount(d, minlength=ecc + 1)
    h = np.float64(0.0)
    for k in range(1, ecc + 1):
        h = h + np.float64(n_d[k]) / np.float64(k)
    return int(d.size), int(d.sum()), ecc, float(h)
