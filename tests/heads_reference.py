"""Plain numpy restatement of the heads contract (the vgl_hip_agg_*_heads calls in include/vgl_hip.h), float64 in entry order with the
sums of absolute terms alongside, built on agg_reference and edge_reference: head h owns the columns [h D, (h + 1) D) of every feature matrix, the
edge scalars are E x H, and every call is its single-head restatement on the head's column slice and the head's column of scalars.  Also the bytes
model of the five calls, term by term."""
import numpy as np

import agg_reference as AR
import edge_reference as ER


def _split(F, H):
    assert H >= 1 and F % H == 0
    D = F // H
    return D, [slice(h * D, (h + 1) * D) for h in range(H)]


def _scalars(t, H=None):
    t = np.asarray(t)
    assert t.ndim == 2 and (H is None or t.shape[1] == H)
    return t


# ---- the five calls ----
def sddmm(rowptr, adj, a, b, H, mean=False):
    """e float32 [E, H], the sum of |a b| per (entry, head) and the unrounded e, float64"""
    a, b = np.asarray(a), np.asarray(b)
    _, cols = _split(a.shape[1], H)
    parts = [ER.sddmm(rowptr, adj, a[:, c], b[:, c], mean=mean) for c in cols]
    return tuple(np.stack([p[k] for p in parts], axis=1) for k in range(3))


def edge_softmax(rowptr, e):
    """y float32 [E, H], the unrounded y, R and d per (entry, head)"""
    e = _scalars(e)
    parts = [ER.edge_softmax(rowptr, e[:, h]) for h in range(e.shape[1])]
    return tuple(np.stack([p[k] for p in parts], axis=1) for k in range(4))


def edge_softmax_backward(rowptr, y, gy):
    """ge float32 [E, H], the unrounded ge and |y| (|gy| + sum |y gy|) per (entry, head)"""
    y, gy = _scalars(y), _scalars(gy)
    parts = [ER.edge_softmax_backward(rowptr, y[:, h], gy[:, h]) for h in range(y.shape[1])]
    return tuple(np.stack([p[k] for p in parts], axis=1) for k in range(3))


def run(rowptr, adj, x, op, w):
    """out float32 [n_rows, F], the sum of |w x| per value and the unrounded out: out[i, f] = the sum over row i of w[p, f // D] x[adj[p], f]"""
    x, w = np.asarray(x), _scalars(w)
    _, cols = _split(x.shape[1], w.shape[1])
    parts = [AR.forward(rowptr, adj, x[:, c], op, w[:, h], with_abs=True) for h, c in enumerate(cols)]
    return tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 2, 3))


def run_transposed(rowptr, adj, n_cols, g, op, w):
    """gx float32 [n_cols, F], the sum of the terms' magnitudes and the unrounded gx"""
    g, w = np.asarray(g), _scalars(w)
    _, cols = _split(g.shape[1], w.shape[1])
    parts = [AR.backward(rowptr, adj, n_cols, g[:, c], op, w[:, h], with_abs=True) for h, c in enumerate(cols)]
    return tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(3))


# ---- float64 gradients ----
def sddmm_backward64(rowptr, adj, n_cols, a, b, ge, H):
    a, b, ge = np.asarray(a), np.asarray(b), _scalars(ge, H)
    _, cols = _split(a.shape[1], H)
    parts = [ER.sddmm_backward64(rowptr, adj, n_cols, a[:, c], b[:, c], ge[:, h]) for h, c in enumerate(cols)]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


def spmm_backward64(rowptr, adj, n_cols, w, x, g, mean=False):
    """(grad w [E, H], grad x [n_cols, F]) of sum(out * g)"""
    w, x, g = _scalars(w), np.asarray(x), np.asarray(g)
    _, cols = _split(x.shape[1], w.shape[1])
    parts = [ER.spmm_backward64(rowptr, adj, n_cols, w[:, h], x[:, c], g[:, c], mean=mean) for h, c in enumerate(cols)]
    return np.stack([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


def softmax_backward64(rowptr, y, gy):
    y, gy = _scalars(y), _scalars(gy)
    return np.stack([ER.softmax_backward64(rowptr, y[:, h], gy[:, h]) for h in range(y.shape[1])], axis=1)


def attention(rowptr, adj, q, k, v, H, scale=None, g=None):
    """attention with H heads: edge_reference.attention per head on the head's slices of q, k and v, scale D ** -0.5 unless given: out [n_rows, Fv],
    w [E, H], bound per value of out and, with g, gq, gk, gv"""
    q, k, v = np.asarray(q), np.asarray(k), np.asarray(v)
    _, qc = _split(q.shape[1], H)
    _, vc = _split(v.shape[1], H)
    parts = [ER.attention(rowptr, adj, q[:, c], k[:, c], v[:, d], scale=scale, g=None if g is None else np.asarray(g)[:, d]) for c, d in zip(qc, vc)]
    res = {key: np.concatenate([p[key] for p in parts], axis=1) for key in ("out", "bound") + (("gq", "gk", "gv") if g is not None else ())}
    res["w"], res["e"] = np.stack([p["w"] for p in parts], axis=1), np.stack([p["e"] for p in parts], axis=1)
    return res


# ---- the shapes and the bytes model ----
def class_entries(rowptr, short=AR.SHORT, wave=AR.WAVE, chunk=AR.CHUNK):
    """the entries of the rows of the short, wave and workgroup class"""
    length = np.diff(np.asarray(rowptr, dtype=np.int64))
    return [int(length[length <= short].sum()), int(length[(length > short) & (length <= wave)].sum()), int(length[length > wave].sum())]


def dot_vec(D):
    return 4 if D % 4 == 0 else 1


def dot_walks(F, H, vec):
    """column_tiles of the heads dot product: per class, the passes over the heads x the tiles of one head"""
    D = F // H
    groups = -(-D // vec)
    walks = []
    for cap in (8, 64, 64):
        nq = 1
        while nq < cap and nq < groups:
            nq *= 2
        hp = 1
        while hp * nq < cap and hp < H:
            hp *= 2
        walks.append(-(-H // hp) * -(-groups // nq))
    return walks


def _lists(rowptr, **switches):
    c = AR.classify(rowptr, **switches)
    return c, 4 * (c["rows_short"] + c["rows_wave"]) + 8 * c["chunks"]


def bytes_sddmm(rowptr, F, H, vec, **switches):
    c, lists = _lists(rowptr, **switches)
    walks = sum(e * t * 4 for e, t in zip(class_entries(rowptr, **switches), dot_walks(F, H, vec)))
    return walks + c["entries"] * 4 * F + c["entries"] * 4 * H + c["rows"] * (8 + 4 * F) + lists


def bytes_softmax(rowptr, H, backward=False, **switches):
    c, lists = _lists(rowptr, **switches)
    return c["entries"] * H * (8 * 2 + 4 if backward else 4 * 3 + 4) + c["rows"] * 8 + lists


def bytes_run(walked_rowptr, F, H, vec, transposed=False, mean=False, **switches):
    """walked_rowptr: the plan's CSR, or its transpose for the transposed run"""
    c, lists = _lists(walked_rowptr, **switches)
    per_entry = 4 + 4 * H + ((4 + (16 if mean else 0)) if transposed else 0)
    walks = sum(e * t * per_entry for e, t in zip(class_entries(walked_rowptr, **switches), AR.column_tiles(F, vec)))
    return walks + c["entries"] * 4 * F + c["rows"] * (8 + 4 * F) + lists
