"""numpy restatement of include/vgl_hip.h's louvain contract: one level of synchronous integer move rounds (move), the run over quotient levels (run)
with every stat and the bytes formula, the simple weighted graph under a list of stored entries, and the fixed graphs of the tests.
Shared by test_louvain_cpu.py and test_louvain_gpu.py; no GPU, no library."""
import numpy as np

import quotient_reference as QR

SHORT, WAVE, WG, CAP_MB = 32, 1024, 4096, 4096        # the defaults of VGL_LOUVAIN_SHORT / _WAVE / _WG / _SORT_CAP_MB
OUTCOMES = ("converged", "reverted", "small_gain", "capped")
M_LIMIT = 1 << 31


def key(i, s):
    """key(i, s) = fmix32(i ^ fmix32(s + 0x9e3779b9)), uint32 arithmetic"""
    mix = QR.fmix32(np.array([(int(s) + 0x9e3779b9) & 0xFFFFFFFF], dtype=np.uint64))[0]
    return QR.fmix32((np.asarray(i, dtype=np.uint64) & np.uint64(0xFFFFFFFF)) ^ mix)


def active(V, seed, r):
    return (key(np.arange(V, dtype=np.uint64), (int(seed) + int(r)) & 0xFFFFFFFF) & np.uint64(1)).astype(bool)


def check_weights(w):
    """m, or ValueError as the library refuses"""
    w = np.asarray(w, dtype=np.int64)
    if len(w) and int(w.min()) < 0:
        raise ValueError("a weight is negative")
    m = int(w.astype(object).sum()) if len(w) else 0
    if m >= M_LIMIT:
        raise ValueError("m is 2^31 or more")
    return m


def move(rowptr, adj, w=None, max_rounds=64, min_gain_den=0, seed=0):
    """one level on the stored CSR (rowptr, adj) as it is.  Returns (labels int32 [V], info): info has m, N (= N_kept), rounds, outcome (a name),
    communities and trace = per evaluated round (N, W, applied before it)"""
    V = len(rowptr) - 1
    rowptr = np.asarray(rowptr, dtype=np.int64)
    adj = np.asarray(adj, dtype=np.int64)
    w = np.ones(len(adj), dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    m = check_weights(w)
    rows = QR.rows_of(rowptr).astype(np.int64)
    k = np.zeros(V, dtype=np.int64)
    np.add.at(k, rows, w)
    nonself = adj != rows
    selfw = int(w[~nonself].sum())
    r_ns, a_ns, w_ns = rows[nonself], adj[nonself], w[nonself]
    comm = np.arange(V, dtype=np.int64)
    kept, n_kept, applied = comm, 0, 0
    trace = []
    r = 0
    while True:
        r += 1
        tot = np.zeros(V, dtype=np.int64)
        np.add.at(tot, comm, k)
        size = np.bincount(comm, minlength=V)
        keys, inverse = np.unique((r_ns << 32) | comm[a_ns], return_inverse=True)
        kvc = np.zeros(len(keys), dtype=np.int64)
        np.add.at(kvc, inverse, w_ns)
        ur, uc = keys >> 32, keys & 0xFFFFFFFF
        own = uc == comm[ur]
        ka = np.zeros(V, dtype=np.int64)
        ka[ur[own]] = kvc[own]
        score_a = ka * m - k * (tot[comm] - k)
        cr, cc, cs = ur[~own], uc[~own], kvc[~own] * m - k[ur[~own]] * tot[uc[~own]]
        order = np.lexsort((cc, -cs, cr))                            # per row: the greatest score first, ties to the smallest id
        cr, cc, cs = cr[order], cc[order], cs[order]
        first = np.ones(len(cr), dtype=bool)
        first[1:] = cr[1:] != cr[:-1]
        best = np.full(V, -1, dtype=np.int64)
        v, b, s = cr[first], cc[first], cs[first]
        wants = (s > score_a[v]) & ~((size[comm[v]] == 1) & (size[b] == 1) & (b > comm[v]))
        best[v[wants]] = b[wants]
        W = int(wants.sum())
        N = m * (int(ka.sum()) + selfw) - int((tot * tot).sum())
        trace.append((N, W, applied))
        if r > 1 and applied > 0 and N <= n_kept:
            outcome, result = "reverted", kept
            break
        before, kept, n_kept, result = n_kept, comm, N, comm
        if min_gain_den > 0 and r > 1 and applied > 0 and N - before < (m * m) // min_gain_den:
            outcome = "small_gain"
            break
        if W == 0:
            outcome = "converged"
            break
        if r == max_rounds:
            outcome = "capped"
            break
        go = (best >= 0) & active(V, seed, r)
        applied = int(go.sum())
        comm = np.where(go, best, comm)
    info = {"m": m, "N": n_kept, "rounds": r, "outcome": outcome, "communities": len(np.unique(result)), "trace": trace}
    return result.astype(np.int32), info


# ---- the simple weighted graph under stored entries ----
def simple_graph(V, src, dst, weights=None):
    """(rowptr, adj, slot weight or None) of the symmetric simple CSR: loops dropped, parallel and antiparallel entries merged; an edge weighs the
    sum of `weights` (per entry of the list) over the entries merged into it"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keep = src != dst
    lo, hi = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep]
    keys, inverse = np.unique((lo << 32) | hi, return_inverse=True)
    lo, hi = keys >> 32, keys & 0xFFFFFFFF
    s, d = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    order = np.lexsort((d, s))
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(s, minlength=V), out=rowptr[1:])
    if weights is None:
        return rowptr, d[order].astype(np.int32), None
    ew = np.zeros(len(keys), dtype=np.int64)
    np.add.at(ew, inverse, np.asarray(weights, dtype=np.int64)[keep])
    return rowptr, d[order].astype(np.int32), np.concatenate([ew, ew])[order]


def class_rows(rowptr, short=SHORT, wave=WAVE, wg=WG):
    return QR.class_rows(np.diff(rowptr), short, wave, wg)


def level_bytes(V, E, rounds, wb):
    return 8 * (V + 1) + (4 + wb) * E + 24 * V + rounds * ((8 + wb) * E + 44 * V) + (rounds - 1) * 32 * V


def run(rowptr, adj, w=None, max_levels=32, max_rounds=64, min_gain_den=0, seed=0, short=SHORT, wave=WAVE, wg=WG, cap_mb=CAP_MB):
    """the run on the level-0 graph (the symmetric simple CSR with its slot weights).  Returns (community int32 [V], levels = the same after every
    level, stats as vgl_hip_louvain_stats without prepared_now, infos = move's info per level)"""
    V0 = len(rowptr) - 1
    if w is not None:
        check_weights(w)
    community = np.arange(V0, dtype=np.int64)
    st = {"levels": 0, "entries_walked": 0, "algorithmic_bytes": 0}
    per = {k: [] for k in ("vertices", "entries", "communities", "level_modularity_num", "rounds", "outcome")}
    lengths = np.diff(rowptr)
    st["rows_short"], st["rows_wave"], st["rows_wg"], st["rows_sorted"] = class_rows(rowptr, short, wave, wg)
    st["sorted_keys"] = int(lengths[lengths > wg].sum())
    st["sort_pieces"] = QR.sort_pieces(lengths, wg, cap_mb)
    levels, infos = [], []
    for l in range(max_levels):
        V, E = len(rowptr) - 1, len(adj)
        labels, info = move(rowptr, adj, w, max_rounds, min_gain_den, (seed + (l << 16)) & 0xFFFFFFFF)
        infos.append(info)
        for k, x in (("vertices", V), ("entries", E), ("communities", info["communities"]), ("level_modularity_num", info["N"]), ("rounds", info["rounds"]),
                     ("outcome", info["outcome"])):
            per[k].append(x)
        st["levels"] = l + 1
        st["entries_walked"] += info["rounds"] * E
        st["algorithmic_bytes"] += level_bytes(V, E, info["rounds"], 0 if w is None else 8)
        st["total_weight"] = infos[0]["m"]
        st["modularity_num"] = info["N"]
        last = info["communities"] == V
        if not last:
            q_rowptr, q_adj, q_count = QR.quotient_dir(rowptr, adj, labels, w, drop_loops=False)
            st["algorithmic_bytes"] += QR.quotient_stats(rowptr, None, labels, len(q_adj), 0)["algorithmic_bytes"] + 8 * V0
            community = QR.vertex_maps(labels)[0].astype(np.int64)[community]
            rowptr, adj, w = q_rowptr, q_adj, q_count
        levels.append(community.astype(np.int32))
        if last:
            break
    st.update(per)
    return community.astype(np.int32), levels, st, infos


def modularity(info_or_stats):
    m = info_or_stats.get("total_weight", info_or_stats.get("m"))
    n = info_or_stats.get("modularity_num", info_or_stats.get("N"))
    return n / (m * m) if m else 0.0


# ---- fixed graphs: name -> (V, src, dst), both directions stored ----
def caveman(caves, n):
    """connected_caveman: `caves` cliques of n in a ring; in every clique the edge (first, second) is rewired to (first, the last of the clique before)"""
    pairs = []
    for c in range(caves):
        base = c * n
        for i in range(n):
            for j in range(i + 1, n):
                if (i, j) != (0, 1):
                    pairs.append((base + i, base + j))
        pairs.append((base, (base - 1) % (caves * n)))
    return (caves * n,) + QR._both(pairs)


def ring_of_cliques(cliques, n):
    pairs = []
    for c in range(cliques):
        base = c * n
        pairs += [(base + i, base + j) for i in range(n) for j in range(i + 1, n)]
        pairs.append((base + 1, ((c + 1) % cliques) * n))
    return (cliques * n,) + QR._both(pairs)


def gnp(V, p, seed):
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(V, 1)
    pick = rng.random(len(iu)) < p
    return (V,) + QR._both(list(zip(iu[pick].tolist(), ju[pick].tolist())))


def grid(n):
    pairs = [(i * n + j, i * n + j + 1) for i in range(n) for j in range(n - 1)] + [(i * n + j, (i + 1) * n + j) for i in range(n - 1) for j in range(n)]
    return (n * n,) + QR._both(pairs)


def petersen():
    return (10,) + QR._both([(i, (i + 1) % 5) for i in range(5)] + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)])


def fixed_graphs():
    g = {}
    g["one_edge"] = (2,) + QR._both([(0, 1)])
    g["matching16"] = (16,) + QR._both([(2 * i, 2 * i + 1) for i in range(8)])
    g["star"] = (9,) + QR._both([(0, i) for i in range(1, 9)])
    g["caveman"] = caveman(8, 6)
    g["ring_of_cliques"] = ring_of_cliques(30, 5)
    g["petersen"] = petersen()
    g["grid12"] = grid(12)
    g["gnp300"] = gnp(300, 0.03, 7)
    g["empty"] = (5, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    return g
