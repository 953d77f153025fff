"""numpy restatement of include/vgl_hip.h's quotient contract: the coarse vertex maps, the coarse entries of one direction with their summed weights, every
stat with its bytes formula, the partition quality figures, an independent brute force over Python dicts and the modularity as an exact Fraction.
Shared by test_quotient_cpu.py and test_quotient_gpu.py; no GPU, no library."""
from fractions import Fraction

import numpy as np

SHORT, WAVE, TABLE, CAP_MB = 32, 1024, 4096, 4096      # the defaults of VGL_QUOT_SHORT / _WAVE / _TABLE / _SORT_CAP_MB
KEY_BYTES = 32                                          # sort buffers per key: key in and out, sum in and out


# ---- hand cases: name -> (V, src, dst), directed entries as stored ----
def _both(pairs):
    s = [a for a, b in pairs] + [b for a, b in pairs]
    d = [b for a, b in pairs] + [a for a, b in pairs]
    return np.array(s, dtype=np.int32), np.array(d, dtype=np.int32)


def two_cliques(n):
    """two disjoint K_n, both directions stored: vertices 0 .. n - 1 and n .. 2n - 1"""
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return (2 * n,) + _both(pairs + [(n + i, n + j) for i, j in pairs])


def hand_cases():
    cases = {}
    cases["path"] = (6,) + _both([(i, i + 1) for i in range(5)])
    cases["star"] = (7,) + _both([(0, i) for i in range(1, 7)])
    cases["k5"] = (5,) + _both([(i, j) for i in range(5) for j in range(i + 1, 5)])
    cases["two_k4"] = two_cliques(4)
    cases["isolated"] = (6,) + _both([(1, 3)])
    s, d = _both([(0, 1), (1, 2)])
    cases["self_loop"] = (3, np.concatenate([s, np.array([1, 1], dtype=np.int32)]), np.concatenate([d, np.array([1, 1], dtype=np.int32)]))
    cases["triple_edge"] = (4, np.array([0, 0, 0, 1, 2, 3, 1], dtype=np.int32), np.array([1, 1, 1, 2, 3, 0, 0], dtype=np.int32))
    cases["directed_cycle"] = (5, np.array([0, 1, 2, 3, 4, 0], dtype=np.int32), np.array([1, 2, 3, 4, 0, 2], dtype=np.int32))
    return cases


def labelings(V):
    """name -> int64 labels in ORIGINAL vertex order"""
    v = np.arange(V, dtype=np.int64)
    sparse = np.array([5, 10 ** 6, 2 ** 31 - 2], dtype=np.int64)
    return {"all_equal": np.full(V, 7, dtype=np.int64), "identity": v, "mod2": v % 2, "non_contiguous": sparse[v % 3]}


# ---- hashing, as the app labels by default ----
def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def hashed_labels(V, K, seed=0):
    return (fmix32(np.arange(V, dtype=np.uint64) ^ np.uint64(seed & 0xFFFFFFFF)) % np.uint64(max(int(K), 1))).astype(np.int64)


# ---- CSR as Graph.from_coo builds it ----
def coo_to_csr(V, src, dst):
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int32)
    perm = np.argsort(src, kind="stable")
    rowptr = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=V), out=rowptr[1:])
    return rowptr, dst[perm].astype(np.int32), perm.astype(np.int64)


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(rowptr))


def build(V, src, dst):
    rowptr, adj, _ = coo_to_csr(V, src, dst)
    in_rowptr, in_adj, _ = coo_to_csr(V, adj, rows_of(rowptr))
    return rowptr, adj, in_rowptr, in_adj


# ---- the coarse vertices ----
def vertex_maps(labels):
    """cluster_of int32 [V], label_of int32 [V'], size int32 [V'], members int32 [V], member_ptr int64 [V' + 1]"""
    labels = np.asarray(labels, dtype=np.int64)
    assert labels.min() >= 0
    label_of, cluster_of, size = np.unique(labels, return_inverse=True, return_counts=True)
    members = np.argsort(cluster_of, kind="stable")
    member_ptr = np.zeros(len(label_of) + 1, dtype=np.int64)
    np.cumsum(size, out=member_ptr[1:])
    return cluster_of.astype(np.int32), label_of.astype(np.int32), size.astype(np.int32), members.astype(np.int32), member_ptr


# ---- the coarse entries of one direction ----
def quotient_dir(rowptr, adj, labels, weights=None, drop_loops=False):
    """(rowptr int64 [V' + 1], adj int32 [E'], count int64 [E']) of the stored CSR (rowptr, adj) under labels in the CSR's own vertex order"""
    cluster_of, label_of = vertex_maps(labels)[:2]
    vc = len(label_of)
    c_row = cluster_of[rows_of(rowptr)].astype(np.int64)
    c_far = cluster_of[adj].astype(np.int64)
    w = np.ones(len(adj), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    if drop_loops:
        keep = c_row != c_far
        c_row, c_far, w = c_row[keep], c_far[keep], w[keep]
    keys, inverse = np.unique((c_row << 32) | c_far, return_inverse=True)
    count = np.zeros(len(keys), dtype=np.int64)
    np.add.at(count, inverse, w)
    out = np.zeros(vc + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys >> 32, minlength=vc), out=out[1:])
    return out, (keys & 0xFFFFFFFF).astype(np.int32), count


def volumes(rowptr, labels):
    """the stored entries of the members of every cluster"""
    cluster_of, label_of = vertex_maps(labels)[:2]
    vol = np.zeros(len(label_of), dtype=np.int64)
    np.add.at(vol, cluster_of, np.diff(rowptr))
    return vol


def class_rows(vol, short=SHORT, wave=WAVE, table=TABLE):
    vol = np.asarray(vol)
    vol = vol[vol > 0]
    return [int((vol <= short).sum()), int(((vol > short) & (vol <= wave)).sum()), int(((vol > wave) & (vol <= table)).sum()), int((vol > table).sum())]


def sort_pieces(vol, table=TABLE, cap_mb=CAP_MB):
    """pieces of consecutive sorted rows whose keys stay under the cap; a row above the cap is a piece of its own"""
    cap = (cap_mb << 20) // KEY_BYTES if cap_mb else None
    pieces, acc = 0, 0
    for v in [int(x) for x in vol if x > table]:
        if cap is not None and acc > 0 and acc + v > cap:
            pieces, acc = pieces + 1, 0
        acc += v
    return pieces + (1 if acc else 0)


def quotient_stats(rowptr, in_rowptr, labels, e_out, e_in, short=SHORT, wave=WAVE, table=TABLE, cap_mb=CAP_MB):
    """vgl_hip_quotient_stats; direction 1 is planned iff there is an incoming CSR (e_in is then its E')"""
    V = len(rowptr) - 1
    vc = len(np.unique(np.asarray(labels)))
    st = {"vertices": vc}
    total = 32 * V + 8 * vc + 8 * (vc + 1)
    for name, rp, e in (("out", rowptr, e_out), ("in", in_rowptr, e_in)):
        if rp is not None:
            vol = volumes(rp, labels)
            r = class_rows(vol, short, wave, table)
            read, skeys, pieces = int(vol.sum()), int(vol[vol > table].sum()), sort_pieces(vol, table, cap_mb)
            total += 28 * V + 40 * (vc + 1) + 16 * read + 12 * int(e)
        else:
            r, read, skeys, pieces, e = [0, 0, 0, 0], 0, 0, 0, 0
        st["rows_short_" + name], st["rows_wave_" + name], st["rows_table_" + name], st["rows_sorted_" + name] = r
        st["entries_read_" + name], st["entries_" + name] = read, int(e)
        st["sorted_keys_" + name], st["sort_pieces_" + name] = skeys, pieces
    st["algorithmic_bytes"] = total
    return st


def quotient_brute(rowptr, adj, labels, weights=None, drop_loops=False):
    """the same rows the slow way: a dict per coarse row, filled entry by entry"""
    distinct = sorted(set(int(x) for x in labels))
    rank = {l: i for i, l in enumerate(distinct)}
    rows = [dict() for _ in distinct]
    for v in range(len(rowptr) - 1):
        c = rank[int(labels[v])]
        for e in range(int(rowptr[v]), int(rowptr[v + 1])):
            cw = rank[int(labels[int(adj[e])])]
            if drop_loops and cw == c:
                continue
            rows[c][cw] = rows[c].get(cw, 0) + (1 if weights is None else int(weights[e]))
    out, a, cnt = [0], [], []
    for r in rows:
        for cw in sorted(r):
            a.append(cw)
            cnt.append(r[cw])
        out.append(len(a))
    return np.array(out, dtype=np.int64), np.array(a, dtype=np.int32), np.array(cnt, dtype=np.int64)


# ---- the quality of a partition ----
def quality(rowptr, adj, labels, weights=None):
    """internal, volume_out, volume_in (int64 [V']), total, cut -- from the stored entries directly, not through the quotient"""
    cluster_of, label_of = vertex_maps(labels)[:2]
    vc = len(label_of)
    w = np.ones(len(adj), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    c_row, c_far = cluster_of[rows_of(rowptr)], cluster_of[adj]
    internal, vout, vin = np.zeros(vc, dtype=np.int64), np.zeros(vc, dtype=np.int64), np.zeros(vc, dtype=np.int64)
    np.add.at(internal, c_row[c_row == c_far], w[c_row == c_far])
    np.add.at(vout, c_row, w)
    np.add.at(vin, c_far, w)
    m = int(w.sum())
    return {"internal": internal, "volume_out": vout, "volume_in": vin, "total": m, "cut": m - int(internal.sum())}


def modularity_fraction(rowptr, adj, labels, weights=None):
    """sum over c of (I_c / m - out_c in_c / m^2), exactly; 0 for m = 0"""
    q = quality(rowptr, adj, labels, weights)
    m = q["total"]
    if m == 0:
        return Fraction(0)
    return sum((Fraction(int(i), m) - Fraction(int(o) * int(n), m * m) for i, o, n in zip(q["internal"], q["volume_out"], q["volume_in"])), Fraction(0))


def modularity_bound(vc):
    """float64 roundings of the device-side formula: a handful per term of magnitude <= 1 and one per addition"""
    return 8 * (vc + 1) * 2.0 ** -53


def random_multigraph(rng, V, E):
    """E stored entries with loops and repeats"""
    src = rng.integers(0, V, size=E).astype(np.int32)
    dst = rng.integers(0, V, size=E).astype(np.int32)
    rep = rng.integers(0, max(E, 1), size=E // 3)
    return np.concatenate([src, src[rep]]), np.concatenate([dst, dst[rep]])
