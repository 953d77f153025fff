"""Plain numpy restatement of the aggregation contract (vgl_hip_agg_* in include/vgl_hip.h): the forward pass of the four ops
with the arg, the transpose, the backward pass, the row classes and chunk counts of the stats, and the derived tolerance.  Sums are taken in
float64, term by term in entry order, and rounded to float32 once at the end."""
import numpy as np

OPS = ("sum", "mean", "max", "min")
SHORT, WAVE, CHUNK, MAX_CHUNKS = 32, 1024, 16384, 32768
U32, U64 = 2.0 ** -24, 2.0 ** -53


def _csr(rowptr, adj):
    rowptr, adj = np.asarray(rowptr, dtype=np.int64), np.asarray(adj, dtype=np.int64)
    length = np.diff(rowptr)
    assert rowptr[0] == 0 and (length >= 0).all() and rowptr[-1] == len(adj)
    return rowptr, adj, length, np.repeat(np.arange(len(length)), length)


def forward(rowptr, adj, x, op, weight=None, with_abs=False):
    """out float32 [n_rows, F], arg int32 [n_rows, F] (None for sum and mean)[, the sum of |c_p v_p| per value and the unrounded result, float64]"""
    rowptr, adj, length, row = _csr(rowptr, adj)
    x = np.asarray(x, dtype=np.float32)
    n, F = len(length), x.shape[1]
    vals = x[adj].astype(np.float64)                                   # E x F
    if op in ("sum", "mean"):
        w = np.ones(len(adj)) if weight is None else np.asarray(weight, dtype=np.float32).astype(np.float64)
        terms = w[:, None] * vals                                      # exact in float64
        acc, mag = np.zeros((n, F)), np.zeros((n, F))
        np.add.at(acc, row, terms)                                     # in entry order
        np.add.at(mag, row, np.abs(terms))
        if op == "mean":
            scale = np.where(length > 0, np.maximum(length, 1), 1).astype(np.float64)[:, None]
            acc, mag = acc / scale, mag / scale
        out = acc.astype(np.float32)
        return (out, None, mag, acc) if with_abs else (out, None)
    assert weight is None, "max and min take no weights"
    sign = -1.0 if op == "min" else 1.0
    out, arg = np.zeros((n, F), dtype=np.float32), np.full((n, F), -1, dtype=np.int32)
    full = np.flatnonzero(length > 0)
    if len(full) and F:
        starts = rowptr[full]
        ext = np.maximum.reduceat(sign * vals, starts, axis=0)          # the non-empty rows are consecutive segments
        at = np.repeat(np.arange(len(full)), length[full])
        pos = np.where(sign * vals == ext[at], np.arange(len(adj))[:, None], np.iinfo(np.int64).max)
        out[full] = (sign * ext).astype(np.float32)
        arg[full] = np.minimum.reduceat(pos, starts, axis=0).astype(np.int32)     # the smallest position that attains it
    return (out, arg, np.abs(out).astype(np.float64), out.astype(np.float64)) if with_abs else (out, arg)


def transpose(rowptr, adj, n_cols):
    """t_rowptr int64 [n_cols + 1], t_row (the row of each transposed entry), origin (its position p): row u lists the entries with adj[p] = u in
    ascending p"""
    rowptr, adj, _, row = _csr(rowptr, adj)
    origin = np.argsort(adj, kind="stable")
    t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(adj, minlength=n_cols))]).astype(np.int64)
    return t_rowptr, row[origin].astype(np.int32), origin.astype(np.int64)


def backward(rowptr, adj, n_cols, g, op, weight=None, arg=None, with_abs=False):
    """gx float32 [n_cols, F] = the sum over the transposed row of u, in its order, of coefficient(p) * g[row(p), :][, the sum of the terms'
    magnitudes and the unrounded result, float64]"""
    rowptr, adj, length, row = _csr(rowptr, adj)
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    F = g.shape[1]
    t_rowptr, t_row, origin = transpose(rowptr, adj, n_cols)
    if op in ("sum", "mean"):
        coef = np.ones(len(adj)) if weight is None else np.asarray(weight, dtype=np.float32).astype(np.float64)
        if op == "mean":
            coef = coef / length[row]
        coef = np.broadcast_to(coef[:, None], (len(adj), F))
    else:
        assert arg is not None and weight is None
        coef = (np.asarray(arg)[row] == np.arange(len(adj))[:, None]).astype(np.float64)
    terms = (coef * g[row])[origin]                                    # in the transposed order
    acc, mag = np.zeros((n_cols, F)), np.zeros((n_cols, F))
    np.add.at(acc, adj[origin], terms)
    np.add.at(mag, adj[origin], np.abs(terms))
    gx = acc.astype(np.float32)
    return (gx, mag, acc) if with_abs else gx


def chunks_of(longest, chunk=CHUNK, max_chunks=MAX_CHUNKS):
    """the chunk of the workgroup rows: the switch's, raised until the longest row has at most max_chunks pieces"""
    longest = max(int(longest), 1)
    return max(int(chunk), -(-longest // max_chunks))


def classify(rowptr, short=SHORT, wave=WAVE, chunk=CHUNK):
    """the plan's stats of a CSR: rows per class (empty rows are short), the workgroup class's chunks, the rows of more than one chunk"""
    length = np.diff(np.asarray(rowptr, dtype=np.int64))
    wg = length[length > wave]
    c = chunks_of(wg.max() if len(wg) else 0, chunk)
    pieces = -(-wg // c)
    return {"rows": int(len(length)), "entries": int(length.sum()), "rows_short": int((length <= short).sum()),
            "rows_wave": int(((length > short) & (length <= wave)).sum()), "rows_wg": int(len(wg)), "chunks": int(pieces.sum()),
            "hub_rows": int((pieces > 1).sum())}


def column_tiles(F, vec):
    """walks per row of the short, wave and workgroup class: a tile is NQ * vec columns, NQ the power of two that covers F up to 8 / 64 / 64 lanes"""
    groups = -(-F // vec)
    tiles = []
    for cap in (8, 64, 64):
        nq = 1
        while nq < cap and nq < groups:
            nq *= 2
        tiles.append(-(-groups // nq))
    return tiles


def tolerance(d):
    """the factor of the sum of |c_p v_p| that bounds |computed - exact| of a value with d terms: gamma_k at u = 2^-24 with k = d + 2 (a rounding per
    product, at most d - 1 additions on a chain, the division of MEAN and the extra product of its backward) plus the restatement's own gamma_k at
    u = 2^-53"""
    k = d + 2
    return k * U32 / (1.0 - k * U32) + k * U64 / (1.0 - k * U64)
