"""Plain numpy restatement of the GAT contract (vgl_hip_agg_edge_add_heads / _edge_sum_heads in include/vgl_hip.h), built on
agg_reference and edge_reference: the additive score in float32 exactly as the contract states it (one addition, one product), the entry sums with
their gate and their transposed forms in float64 in the order of the contract with the sums of |c| alongside, GAT attention and every gradient in
float64, and the bytes model of the two calls term by term.  s is n_rows x H, t n_cols x H, the entry scalars E x H."""
import numpy as np

import agg_reference as AR
import edge_reference as ER

U32, U64 = AR.U32, AR.U64


def row_index(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def _two(x):
    x = np.asarray(x)
    return x[:, None] if x.ndim == 1 else x


# ---- the score ----
def score(rowptr, adj, s, t, slope):
    """e float32 [E, H]: z = s[row] + t[adj] (np.float32 addition; a term that is None is absent, nothing is added), e = z > 0 ? z : slope * z (one
    np.float32 product)"""
    row, adj = row_index(rowptr), np.asarray(adj, dtype=np.int64)
    assert s is not None or t is not None
    if s is None:
        z = _two(np.asarray(t, dtype=np.float32))[adj]
    elif t is None:
        z = _two(np.asarray(s, dtype=np.float32))[row]
    else:
        z = _two(np.asarray(s, dtype=np.float32))[row] + _two(np.asarray(t, dtype=np.float32))[adj]
    assert z.dtype == np.float32
    return np.where(z > 0, z, np.float32(slope) * z).astype(np.float32)


# ---- the sums ----
def gated(w, gate, slope):
    """c float64 [E, H]: w, or slope * w where a gate is given and is not above 0; the product of two float32 is exact in float64"""
    w = _two(np.asarray(w, dtype=np.float32)).astype(np.float64)
    if gate is None:
        return w
    return np.where(_two(np.asarray(gate, dtype=np.float32)) > 0, w, float(np.float32(slope)) * w)


def edge_sum(rowptr, adj, n_cols, w, gate=None, slope=1.0, transposed=False):
    """out float32 [rows, H], the sum of |c| per value, the unrounded out (float64) and the terms d per row: over the entries of row i in order, or
    with transposed over the entries with adj[p] = u in ascending p"""
    c = gated(w, gate, slope)
    adj = np.asarray(adj, dtype=np.int64)
    if transposed:
        _, _, origin = AR.transpose(rowptr, adj, n_cols)
        to, c, n = adj[origin], c[origin], n_cols
    else:
        to, n = row_index(rowptr), len(rowptr) - 1
    acc, mag = np.zeros((n, c.shape[1])), np.zeros((n, c.shape[1]))
    np.add.at(acc, to, c)                                              # in the order of the walk
    np.add.at(mag, to, np.abs(c))
    return acc.astype(np.float32), mag, acc, np.bincount(to, minlength=n)


def sum_bound(d):
    """the factor of the sum of |c|: one rounding for the product of a gated term and at most d - 1 additions on a chain whatever the shape: gamma_k,
    k = d, at u = 2^-24, plus the restatement's own d - 1 additions at u = 2^-53"""
    d = np.asarray(d, dtype=np.float64)
    return ER.gamma(d) + ER.gamma(d, U64)


# ---- float64 gradients ----
def score64(rowptr, adj, s, t, slope):
    z = _two(np.asarray(s, dtype=np.float64))[row_index(rowptr)] + _two(np.asarray(t, dtype=np.float64))[np.asarray(adj, dtype=np.int64)]
    return np.where(z > 0, z, float(slope) * z)


def score_backward64(rowptr, adj, n_cols, e, ge, slope):
    """(grad s [n_rows, H], grad t [n_cols, H]) of sum(e * ge): the derivative of the activation is 1 where e > 0 and slope elsewhere (torch's)"""
    c = np.where(_two(np.asarray(e)) > 0, 1.0, float(slope)) * _two(np.asarray(ge, dtype=np.float64))
    gs, gt = np.zeros((len(rowptr) - 1, c.shape[1])), np.zeros((n_cols, c.shape[1]))
    np.add.at(gs, row_index(rowptr), c)
    np.add.at(gt, np.asarray(adj, dtype=np.int64), c)
    return gs, gt


def attention(rowptr, adj, s, t, v, slope, g=None):
    """GAT attention with H = s.shape[1] heads, float64: out [n_rows, Fv], w [E, H], e [E, H] and, with a gradient g of out, gs, gt, gv; per head it
    is edge_reference's softmax64 / spmm64 on the head's column of the score and the head's slice of v.  `bound` per value of out, for out computed
    in float32 from the float32 s, t, v as in edge_reference.attention: the score carries eta = gamma_2 |e| (two roundings), a weight
    rel = expm1(2 eta) + exp(2 eta) (softmax_bound(d, R + 2 eta) + u), the weighted sum gamma_(d + 2)."""
    s, t, v = _two(np.asarray(s, dtype=np.float32)), _two(np.asarray(t, dtype=np.float32)), np.asarray(v, dtype=np.float32)
    rowptr, adj = np.asarray(rowptr, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    row, length = row_index(rowptr), np.diff(rowptr)
    n, n_cols, H = len(length), v.shape[0], s.shape[1]
    D = v.shape[1] // H
    assert v.shape[1] == H * D
    e = score64(rowptr, adj, s, t, slope)
    w = np.stack([ER.softmax64(rowptr, e[:, h]) for h in range(H)], axis=1)
    res = {"e": e, "w": w}
    out, bound = [], []
    d = int(length.max(initial=0))
    tol = AR.tolerance(d)
    for h in range(H):
        x = v[:, h * D:(h + 1) * D].astype(np.float64)
        o, omag = ER.spmm64(rowptr, adj, w[:, h], x)
        eta = np.zeros(n)
        np.maximum.at(eta, row, ER.gamma(2) * np.abs(e[:, h]))
        m = np.full(n, -np.inf)
        np.maximum.at(m, row, e[:, h])
        R = np.zeros(n)
        np.maximum.at(R, row, m[row] - e[:, h])
        rel = np.expm1(2 * eta) + np.exp(2 * eta) * (ER.softmax_bound(length, R + 2 * eta) + U32)
        out.append(o)
        bound.append((rel * (1 + tol) + tol)[:, None] * omag + length[:, None] * ER.TINY * np.abs(x).max(initial=0.0))
    res["out"], res["bound"] = np.concatenate(out, axis=1), np.concatenate(bound, axis=1)
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        gw, gv = [], []
        for h in range(H):
            a, b = ER.spmm_backward64(rowptr, adj, n_cols, w[:, h], v[:, h * D:(h + 1) * D].astype(np.float64), g[:, h * D:(h + 1) * D])
            gw.append(a)
            gv.append(b)
        ge = np.stack([ER.softmax_backward64(rowptr, w[:, h], gw[h]) for h in range(H)], axis=1)
        res["gv"] = np.concatenate(gv, axis=1)
        res["gs"], res["gt"] = score_backward64(rowptr, adj, n_cols, e, ge, slope)
    return res


# ---- the bytes model ----
def _lists(rowptr, **switches):
    c = AR.classify(rowptr, **switches)
    return c, 4 * (c["rows_short"] + c["rows_wave"]) + 8 * c["chunks"]


def bytes_score(rowptr, H, has_s=True, has_t=True, **switches):
    """entries x (4 adjacency + 4 H of t when present + 4 H written) + rows x (8 + 4 H of s when present) + the list entries"""
    c, lists = _lists(rowptr, **switches)
    return c["entries"] * (4 + (4 * H if has_t else 0) + 4 * H) + c["rows"] * (8 + (4 * H if has_s else 0)) + lists


def bytes_sum(walked_rowptr, H, gate=False, transposed=False, **switches):
    """walked_rowptr: the plan's CSR, or its transpose.  entries x (4 H + 4 H with a gate + 4 of the origin when transposed) + rows x (8 + 4 H
    written) + the list entries"""
    c, lists = _lists(walked_rowptr, **switches)
    return c["entries"] * (4 * H * (2 if gate else 1) + (4 if transposed else 0)) + c["rows"] * (8 + 4 * H) + lists


def head_block(H):
    return 8 if H % 8 == 0 else 4 if H % 4 == 0 else 2 if H % 2 == 0 else 1


def vec_of(H, wide=True):
    """the vec of the stats: 4 where a lane's block of heads moves in 16-byte pieces"""
    return 4 if wide and head_block(H) >= 4 else 1
