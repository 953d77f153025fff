"""Restatement of the maximal independent set / maximal matching contract of include/vgl_hip.h (vgl_hip_mis_run, vgl_hip_matching_run).

The definition is the sequential greedy algorithm: greedy_mis_sequential takes the vertices ascending by (priority, id) and keeps a vertex iff none
of its neighbours is kept; greedy_matching_sequential takes the edges ascending by (priority, edge id) and keeps an edge iff both ends are free.
mis_rounds / matching_rounds restate the synchronous rounds of the contract in numpy (usable at scale); they return the same sets -- Blelloch,
Fineman, Shun, SPAA 2012 -- and, beyond them, the per-vertex rounds and the statistics rounds, live_total and entries_walked.  None of this is the
library's method: no row classes, no worklists, no early exit."""
import numpy as np

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def fmix32(h):
    """the murmur3 finaliser on uint32 values"""
    h = np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def key(ids, seed=0):
    """key(i, seed) = fmix32(i ^ fmix32(seed + 0x9e3779b9)), uint32 values as a uint64 array"""
    mix = fmix32(np.uint64((int(seed) + 0x9e3779b9) & 0xFFFFFFFF))
    return fmix32((np.asarray(ids, dtype=np.uint64) & np.uint64(0xFFFFFFFF)) ^ mix)


def simple_graph(V, src, dst):
    """the simple undirected graph under the stored entries: the edges (lo < hi, ascending (lo, hi): the library's numbering) and the symmetric CSR with
    rows ascending and the edge of every slot.  Returns dict(V, eu, ev, rowptr, adj, eid, row, deg)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keep = src != dst
    lo, hi = np.minimum(src[keep], dst[keep]), np.maximum(src[keep], dst[keep])
    code = np.unique(lo * max(V, 1) + hi)
    eu, ev = code // max(V, 1), code % max(V, 1)
    E = eu.size
    row = np.concatenate([eu, ev])
    adj = np.concatenate([ev, eu])
    eid = np.concatenate([np.arange(E), np.arange(E)])
    order = np.lexsort((adj, row))
    row, adj, eid = row[order], adj[order], eid[order]
    deg = np.bincount(row, minlength=V).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return {"V": V, "eu": eu, "ev": ev, "rowptr": rowptr, "adj": adj, "eid": eid, "row": row, "deg": deg}


def _rank(prio):
    """position of every item in the order ascending (priority, id)"""
    prio = np.asarray(prio, dtype=np.uint64)
    order = np.lexsort((np.arange(prio.size), prio))
    rank = np.empty(prio.size, dtype=np.int64)
    rank[order] = np.arange(prio.size)
    return order, rank


def greedy_mis_sequential(G, prio):
    """THE DEFINITION: bool [V]"""
    order, _ = _rank(prio)
    rowptr, adj = G["rowptr"], G["adj"]
    in_set = np.zeros(G["V"], dtype=bool)
    for v in order.tolist():
        if not in_set[adj[rowptr[v]:rowptr[v + 1]]].any():
            in_set[v] = True
    return in_set


def greedy_matching_sequential(G, eprio):
    """THE DEFINITION: (bool [E'], mate int64 [V])"""
    order, _ = _rank(eprio)
    eu, ev = G["eu"], G["ev"]
    mate = np.full(G["V"], -1, dtype=np.int64)
    mask = np.zeros(eu.size, dtype=bool)
    for e in order.tolist():
        a, b = int(eu[e]), int(ev[e])
        if mate[a] < 0 and mate[b] < 0:
            mate[a], mate[b], mask[e] = b, a, True
    return mask, mate


def mis_rounds(G, prio):
    """the synchronous rounds of the contract: dict(in_set bool [V], round int32 [V], rounds, set_size, live_total, entries_walked)"""
    V, deg = G["V"], G["deg"]
    _, rank = _rank(prio)
    before = rank[G["adj"]] < rank[G["row"]]                      # the entries whose far end comes before the row's vertex
    row, adj = G["row"][before], G["adj"][before]
    state = np.zeros(V, dtype=np.int64)
    rounds = live_total = walked = 0
    while True:
        live = state == 0
        n = int(live.sum())
        if n == 0:
            break
        rounds += 1
        live_total += n
        walked += int(deg[live].sum())
        sel = live[row]
        row, adj = row[sel], adj[sel]                             # (a decided row never comes back)
        s = state[adj]                                            # every decision read here is of a round < this one
        has_in = np.bincount(row[s > 0], minlength=V) > 0
        blocked = np.bincount(row[s == 0], minlength=V) > 0
        out = live & has_in
        inn = live & ~has_in & ~blocked
        state[out] = -rounds
        state[inn] = rounds
    return {"in_set": state > 0, "round": state.astype(np.int32), "rounds": rounds, "set_size": int((state > 0).sum()), "live_total": live_total,
            "entries_walked": walked}


def matching_rounds(G, eprio):
    """the two-pass rounds of the contract: dict(in_matching bool [E'], mate int32 [V], round int32 [V], rounds, matched_edges, matched_vertices,
    undirected_edges, live_total, entries_walked)"""
    V, deg, eu, ev = G["V"], G["deg"], G["eu"], G["ev"]
    E = eu.size
    k64 = (np.asarray(eprio, dtype=np.uint64) << np.uint64(32)) | np.arange(E, dtype=np.uint64)
    ekey = k64[G["eid"]]
    order = np.lexsort((ekey, G["row"]))                          # rows ascending, the smallest key of a row first
    row, adj, ekey = G["row"][order], G["adj"][order], ekey[order]
    mate = np.full(V, -1, dtype=np.int64)
    rnd = np.zeros(V, dtype=np.int64)
    mask = np.zeros(E, dtype=bool)
    live = np.ones(V, dtype=bool)
    rounds = live_total = walked = 0
    while live.any():
        rounds += 1
        live_total += int(live.sum())
        walked += int(deg[live].sum())
        sel = (mate[row] < 0) & (mate[adj] < 0)
        row, adj, ekey = row[sel], adj[sel], ekey[sel]            # (a matched end never comes back)
        at = np.flatnonzero(live[row])
        rows, first = np.unique(row[at], return_index=True)       # pass 1: the vertices with a best, and their best
        best = np.full(V, NONE, dtype=np.uint64)
        best[rows] = ekey[at[first]]
        e = (best[rows] & np.uint64(0xFFFFFFFF)).astype(np.int64)  # pass 2
        far = np.where(eu[e] == rows, ev[e], eu[e])
        hit = best[far] == best[rows]
        mate[rows[hit]] = far[hit]
        rnd[rows[hit]] = rounds
        mask[e[hit]] = True
        live = np.zeros(V, dtype=bool)
        live[rows[~hit]] = True
    m = int(mask.sum())
    return {"in_matching": mask, "mate": mate.astype(np.int32), "round": rnd.astype(np.int32), "rounds": rounds, "matched_edges": m, "matched_vertices": 2 * m,
            "undirected_edges": int(E), "live_total": live_total, "entries_walked": walked}


def algorithmic_bytes(kind, V, nnz, live_total, entries_walked, rounds, in_set=True, edges=True, in_matching=True, round=True):
    """the header's bytes models, term by term; nnz = 2 E' entries of the symmetric CSR"""
    if V == 0:
        return 0
    if kind == "mis":
        return 12 * V + 24 * live_total + 8 * entries_walked + 64 * (rounds + 1) + (5 * V if in_set else 0)
    E = nnz // 2
    return 20 * V + 28 * live_total + 12 * entries_walked + 72 * (rounds + 1) + (16 * E if edges else 0) + (E if in_matching else 0) + (4 * V if round else 0)


MIS_STATS = ("rounds", "set_size", "live_total", "entries_walked")
MATCHING_STATS = ("rounds", "matched_edges", "matched_vertices", "undirected_edges", "live_total", "entries_walked")


def _complete(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


TEAM_EDGE_BOUNDS = (4, 20)                                                       # VGL_MIS_SHORT, VGL_MIS_WAVE of the graph below
TEAM_EDGE_ROWS = (33, 5, 2)                                                      # its rows per class under those bounds


def rows_at_the_team_edges():
    """(V, src, dst) of 40 vertices whose rows fill the classes under TEAM_EDGE_BOUNDS to one item past a full workgroup of the kernels: 33 short rows
    (32 per workgroup + 1), 5 wave rows (4 + 1), 2 workgroup rows; the row lengths sit on the bounds: 0 (vertex 7, isolated) and 4 among the short
    rows, 5 and 20 among the wave rows, 21 for a workgroup row.  A graph of 40 vertices cannot hold a row longer than 39: hence the small wave bound.
    Vertices 0, 1: workgroup rows (21, 25 entries); 2 .. 6: wave rows (5, 20, 6, 7, 8); 8 .. 39: short rows that the hubs share out in turn (2 or 3
    each), two of them joined to make a row of exactly 4."""
    shrt, wave = TEAM_EDGE_BOUNDS
    hubs = {0: wave + 1, 1: wave + 5, 2: shrt + 1, 3: wave, 4: shrt + 2, 5: shrt + 3, 6: shrt + 4}
    leaves = np.arange(8, 40)
    src, dst, at = [], [], 0
    for h, d in hubs.items():
        src.append(np.full(d, h))
        dst.append(leaves[(at + np.arange(d)) % leaves.size])
        at += d
    hits = np.bincount(np.concatenate(dst), minlength=40)
    a, b = np.flatnonzero(hits == 3)[:2]                                         # two leaves of three hubs each: one more entry makes 4
    src.append(np.array([a, 8]))                                                 # (and a stored duplicate of an entry, a loop: the simple graph drops them)
    dst.append(np.array([b, 8]))
    return 40, np.concatenate(src), np.concatenate(dst)


# name -> (V, stored entries, vertex priorities, edge priorities (one per undirected edge, ascending (lo, hi)), expected set, expected matching)
HAND_CASES = {
    "empty": (0, [], [], [], [], []),
    "isolated_vertices": (4, [], [3, 1, 2, 0], [], [0, 1, 2, 3], []),
    "only_loops": (3, [(0, 0), (1, 1), (2, 2), (1, 1)], [5, 5, 5], [], [0, 1, 2], []),
    "one_edge_stored_three_times": (2, [(0, 1), (1, 0), (0, 1), (1, 0), (0, 1), (1, 0)], [9, 4], [7], [1], [(0, 1)]),
    # order of the vertices 1, 3, 0, 5, 2, 4; of the edges (1,2), (3,4), (4,5), (0,1), (2,3)
    "path_6": (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)], [2, 0, 4, 1, 5, 3], [3, 0, 4, 1, 2], [1, 3, 5], [(1, 2), (3, 4)]),
    # edges (0,1), (0,5), (1,2), (2,3), (3,4), (4,5) taken in reverse
    "cycle_6": (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0)], [0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [0, 2, 4], [(0, 1), (2, 3), (4, 5)]),
    # vertex 2 first; edge 6 = (1,4) first, then edge 7 = (2,3)
    "k5": (5, _complete(5), [4, 3, 0, 1, 2], [9, 8, 7, 6, 5, 4, 0, 3, 2, 1], [2], [(1, 4), (2, 3)]),
    # the hub last; edge 3 = (0,4) first
    "star_8": (9, [(0, i) for i in range(1, 9)], [8, 0, 1, 2, 3, 4, 5, 6, 7], [3, 1, 4, 0, 5, 9, 2, 6], [1, 2, 3, 4, 5, 6, 7, 8], [(0, 4)]),
    # edges (0,3), (0,4), (0,5), (1,3), (1,4), (1,5), (2,3), (2,4), (2,5): (0,4), (1,3), then (1,5) is blocked, (2,5)
    "k33": (6, [(a, b) for a in range(3) for b in range(3, 6)], [1, 2, 0, 5, 4, 3], [4, 0, 8, 1, 5, 2, 6, 7, 3], [0, 1, 2], [(0, 4), (1, 3), (2, 5)]),
    # triangles 0-1-2 and 2-3-4: vertices 0, 2, 1, 4, 3; edges (0,1), (0,2), (1,2), (2,3), (2,4), (3,4) in the order (0,2), (1,2), (0,1), (3,4)
    "bowtie": (5, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 2)], [0, 2, 1, 4, 3], [2, 0, 1, 5, 4, 3], [0, 4], [(0, 2), (3, 4)]),
}


def hand_case(name):
    """(G, vertex priorities, edge priorities, expected in_set bool [V], expected in_matching bool [E'])"""
    V, stored, vprio, eprio, want_set, want_match = HAND_CASES[name]
    G = simple_graph(V, [a for a, _ in stored], [b for _, b in stored])
    edges = list(zip(G["eu"].tolist(), G["ev"].tolist()))
    assert len(eprio) == len(edges) and len(vprio) == V, name
    in_set = np.zeros(V, dtype=bool)
    in_set[want_set] = True
    mask = np.array([e in want_match for e in edges], dtype=bool)
    assert int(mask.sum()) == len(want_match), name
    return G, np.asarray(vprio, dtype=np.uint64), np.asarray(eprio, dtype=np.uint64), in_set, mask
