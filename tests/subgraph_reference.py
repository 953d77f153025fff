"""numpy restatement of include/vgl_hip.h's subgraph contract: the stable row filter (vertex mask, entry mask), bounded multi-seed reach, fixed-fanout
sampling by priority key, sample_blocks, and every stat and bytes formula.  Shared by test_subgraph_cpu.py and test_subgraph_gpu.py; no GPU, no library."""
import numpy as np

SHORT, WAVE = 32, 1024                   # the default class bounds (VGL_SUB_* / VGL_SAMPLE_*)


# ---- hand cases: name -> (V, src, dst), directed entries as stored ----
def _both(pairs):
    s = [a for a, b in pairs] + [b for a, b in pairs]
    d = [b for a, b in pairs] + [a for a, b in pairs]
    return np.array(s, dtype=np.int32), np.array(d, dtype=np.int32)


def hand_cases():
    cases = {}
    cases["path"] = (6,) + _both([(i, i + 1) for i in range(5)])
    cases["star"] = (7,) + _both([(0, i) for i in range(1, 7)])
    cases["k5"] = (5,) + _both([(i, j) for i in range(5) for j in range(i + 1, 5)])
    cases["two_components"] = (7,) + _both([(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 6)])
    cases["isolated"] = (6,) + _both([(1, 3)])
    s, d = _both([(0, 1), (1, 2)])
    cases["self_loop"] = (3, np.concatenate([s, np.array([1], dtype=np.int32)]), np.concatenate([d, np.array([1], dtype=np.int32)]))
    cases["triple_edge"] = (4, np.array([0, 0, 0, 1, 2, 3, 1], dtype=np.int32), np.array([1, 1, 1, 2, 3, 0, 0], dtype=np.int32))
    return cases


# ---- CSR as Graph.from_coo builds it ----
def coo_to_csr(V, src, dst):
    """stable COO -> CSR; returns rowptr (int64), adj (int32), perm (int64: the input index of every CSR position)"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int32)
    perm = np.argsort(src, kind="stable")
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=rowptr[1:])
    return rowptr, dst[perm].astype(np.int32), perm.astype(np.int64)


def rows_of(rowptr):
    """the row of every CSR position"""
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(rowptr))


def transpose(V, rowptr, adj):
    """the incoming CSR of from_coo: the stable build over the transposed list taken in outgoing CSR order"""
    r, a, _ = coo_to_csr(V, adj, rows_of(rowptr))
    return r, a


def build(V, src, dst):
    rowptr, adj, _ = coo_to_csr(V, src, dst)
    in_rowptr, in_adj = transpose(V, rowptr, adj)
    return rowptr, adj, in_rowptr, in_adj


# ---- the filter ----
def vertex_maps(V, keep_vertex):
    keep = np.ones(V, dtype=bool) if keep_vertex is None else np.asarray(keep_vertex) != 0
    new_id = np.where(keep, np.cumsum(keep) - keep, -1).astype(np.int32)
    return new_id, np.nonzero(keep)[0].astype(np.int32)


def filter_rows(rowptr, adj, keep_vertex=None, keep_entry=None):
    """one direction: (new rowptr int64, new adj int32, origin int64, new_id, old_id)"""
    V = len(rowptr) - 1
    new_id, old_id = vertex_maps(V, keep_vertex)
    row = rows_of(rowptr)
    ok = (new_id[row] >= 0) & (new_id[adj] >= 0)
    if keep_entry is not None:
        ok &= np.asarray(keep_entry) != 0
    origin = np.nonzero(ok)[0].astype(np.int64)
    out = np.zeros(len(old_id) + 1, dtype=np.int64)
    np.cumsum(np.bincount(new_id[row[origin]], minlength=len(old_id)), out=out[1:])
    return out, new_id[adj[origin]].astype(np.int32), origin, new_id, old_id


def class_rows(lengths, short=SHORT, wave=WAVE):
    lengths = np.asarray(lengths)
    return [int((lengths <= short).sum()), int(((lengths > short) & (lengths <= wave)).sum()), int((lengths > wave).sum())]


def filter_stats(rowptr, adj, in_rowptr, in_adj, keep_vertex=None, keep_entry=None, short=SHORT, wave=WAVE):
    """vgl_hip_subgraph_stats; direction 1 is planned iff there is an incoming CSR and no entry mask"""
    V = len(rowptr) - 1
    new_id, old_id = vertex_maps(V, keep_vertex)
    vk = len(old_id)
    st = {"vertices_kept": vk}
    me = 0 if keep_entry is None else 1
    total = (V if keep_vertex is not None else 0) + 4 * V + 4 * vk
    for name, rp, ad, planned in (("out", rowptr, adj, True), ("in", in_rowptr, in_adj, in_rowptr is not None and keep_entry is None)):
        if planned:
            lens = np.diff(rp)[old_id]
            r = class_rows(lens, short, wave)
            read = int(lens.sum())
            kept = len(filter_rows(rp, ad, keep_vertex, keep_entry if name == "out" else None)[1]) if vk else 0
            total += 56 * vk + 32 * (vk + 1) + (16 + 2 * me) * read + 4 * kept
        else:
            r, read, kept = [0, 0, 0], 0, 0
        st["rows_short_" + name], st["rows_wave_" + name], st["rows_wg_" + name] = r
        st["entries_read_" + name], st["entries_kept_" + name] = read, kept
    st["algorithmic_bytes"] = total
    return st


def filter_brute(V, rowptr, adj, keep_vertex=None, keep_entry=None):
    """the same subgraph the slow way: walk the stored entries in CSR order, keep the edge list, rebuild both directions as from_coo does"""
    keep = [True] * V if keep_vertex is None else [bool(x) for x in keep_vertex]
    new_id, nxt = [], 0
    for v in range(V):
        new_id.append(nxt if keep[v] else -1)
        nxt += keep[v]
    src, dst, origin = [], [], []
    for v in range(V):
        for e in range(int(rowptr[v]), int(rowptr[v + 1])):
            w = int(adj[e])
            if keep[v] and keep[w] and (keep_entry is None or keep_entry[e]):
                src.append(new_id[v]); dst.append(new_id[w]); origin.append(e)
    return (nxt,) + build(nxt, np.array(src, dtype=np.int32), np.array(dst, dtype=np.int32)) + (np.array(origin, dtype=np.int64),)


# ---- bounded multi-seed reach ----
def k_hop(rowptr, adj, in_rowptr, in_adj, seeds, hops, direction=0, symmetric=False):
    """(hop int32 [V], stats of vgl_hip_khop_stats)"""
    V = len(rowptr) - 1
    follow = []
    if symmetric or direction == 0:
        follow.append((rowptr, adj))
    if symmetric or direction == 1:
        follow.append((in_rowptr, in_adj))
    hop = np.full(V, -1, dtype=np.int32)
    seeds = np.asarray(seeds, dtype=np.int64)
    hop[seeds] = 0
    st = {"levels_run": 0, "frontier_total": 0, "edges_examined": 0}
    front = np.unique(seeds)
    level = 0
    while level < hops and len(front):
        st["levels_run"] += 1
        st["frontier_total"] += len(front)
        found = []
        for rp, ad in follow:
            st["edges_examined"] += int((rp[front + 1] - rp[front]).sum())
            for v in front:
                found.append(ad[rp[v]:rp[v + 1]])
        found = np.unique(np.concatenate(found)) if found else np.zeros(0, dtype=np.int64)
        front = found[hop[found] < 0].astype(np.int64)
        hop[front] = level + 1
        level += 1
    st["reached"] = int((hop >= 0).sum())
    return hop, st


def k_hop_brute(V, src, dst, seeds, hops, direction=0, symmetric=False):
    """Bellman-Ford over the edge list, hops rounds at most"""
    edges = []
    if symmetric or direction == 0:
        edges += list(zip(src.tolist(), dst.tolist()))
    if symmetric or direction == 1:
        edges += list(zip(dst.tolist(), src.tolist()))
    big = 1 << 40
    d = [big] * V
    for s in seeds:
        d[s] = 0
    for _ in range(min(int(hops), V)):
        nd = list(d)
        for u, v in edges:
            if d[u] + 1 < nd[v]:
                nd[v] = d[u] + 1
        if nd == d:
            break
        d = nd
    return np.array([x if x <= hops and x < big else -1 for x in d], dtype=np.int32)


# ---- sampling ----
def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def key(ids, seed):
    """api.priority_key: key(i, seed) = fmix32(i ^ fmix32(seed + 0x9e3779b9))"""
    mix = fmix32(np.array([(int(seed) + 0x9e3779b9) & 0xFFFFFFFF], dtype=np.uint64))[0]
    return fmix32((np.asarray(ids, dtype=np.uint64) & 0xFFFFFFFF) ^ mix)


def sample(rowptr, adj, seeds, fanout, seed, short=SHORT, wave=WAVE):
    """(rowptr int64 [n + 1], adj int32, origin int64, stats of vgl_hip_sample_stats)"""
    seeds = np.asarray(seeds, dtype=np.int64)
    n = len(seeds)
    out, org = [np.zeros(0, dtype=np.int64)], np.zeros(n + 1, dtype=np.int64)
    for i, v in enumerate(seeds):
        p = np.arange(rowptr[v], rowptr[v + 1], dtype=np.int64)
        if len(p) > fanout:
            p = np.sort(p[np.argsort(key(p, seed), kind="stable")[:fanout]])
        out.append(p)
        org[i + 1] = org[i] + len(p)
    origin = np.concatenate(out)
    deg = rowptr[seeds + 1] - rowptr[seeds] if n else np.zeros(0, dtype=np.int64)
    r = class_rows(deg, short, wave)
    total = int(org[n])
    st = {"seeds": n, "rows_short": r[0], "rows_wave": r[1], "rows_wg": r[2], "entries_examined": int(deg.sum()), "sampled_total": total,
          "algorithmic_bytes": 60 * n + 16 * (n + 1) + 8 * total}
    return org, adj[origin].astype(np.int32), origin, st


def sample_brute(rowptr, adj, seeds, fanout, seed):
    """sort of (key, position), take fanout, sort by position -- in plain Python integers"""
    def f(h):
        h ^= h >> 16; h = (h * 0x85ebca6b) & 0xFFFFFFFF; h ^= h >> 13; h = (h * 0xc2b2ae35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    mix = f((int(seed) + 0x9e3779b9) & 0xFFFFFFFF)
    rows = []
    for v in seeds:
        ps = list(range(int(rowptr[v]), int(rowptr[v + 1])))
        chosen = sorted(p for _, p in sorted((f((p & 0xFFFFFFFF) ^ mix), p) for p in ps)[:fanout])
        rows.append([(p, int(adj[p])) for p in chosen])
    return rows


def sample_blocks(rowptr, adj, seeds, fanouts, seed):
    """one (frontier, rowptr, adj) per hop: hop h samples with seed + h; the next frontier is the sorted unique union of the frontier and its samples"""
    front = np.asarray(seeds, dtype=np.int32)
    blocks = []
    for h, fanout in enumerate(fanouts):
        rp, ad, _, _ = sample(rowptr, adj, front, fanout, seed + h)
        blocks.append((front, rp, ad))
        front = np.unique(np.concatenate([front, ad])).astype(np.int32)
    return blocks


# ---- triangles of the simple undirected graph under a CSR (for the composition test) ----
def triangle_count(V, rowptr, adj):
    row = rows_of(rowptr).astype(np.int64)
    a = adj.astype(np.int64)
    m = row != a
    lo, hi = np.minimum(row[m], a[m]), np.maximum(row[m], a[m])
    e = np.unique(lo * V + hi)
    lo, hi = e // V, e % V
    nb = [set() for _ in range(V)]
    for u, v in zip(lo.tolist(), hi.tolist()):
        nb[u].add(v)
    return sum(len(nb[u] & nb[v]) for u, v in zip(lo.tolist(), hi.tolist()))
