"""Plain numpy restatement of the edge contract (vgl_hip_agg_sddmm / _edge_softmax / _edge_softmax_backward in include/vgl_hip.h):
the dot product per stored entry, the softmax over each row's entries with its -inf rules, its backward, dot-product attention and every gradient of
them, all in float64 in entry order with the sums of absolute terms alongside, and the derived bounds."""
import numpy as np

import agg_reference as AR

U32, U64 = AR.U32, AR.U64
# The largest error of the device expf against float64 exp over every float32 in [-17, -2^-24] and at 0, in ulps of the result, as
# tests/studies/expf_ulps.hip measured it (DESIGN section 30 has the sweep), plus one ulp because the library's call is compiled in another
# translation unit.
EXP_ULPS_MEASURED = 0.857                        # 0.856681 at x = -5.28543615, over 235 405 314 arguments
EXP_ULPS = EXP_ULPS_MEASURED + 1.0
EPS_EXP = EXP_ULPS * 2.0 ** -23                  # an ulp is at most 2^-23 of the value
TINY = 2.0 ** -126                               # below it float32 is subnormal: an absolute term


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def _rows(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    length = np.diff(rowptr)
    assert rowptr[0] == 0 and (length >= 0).all()
    return rowptr, length, np.repeat(np.arange(len(length)), length)


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _row_sum(row, n, terms):
    acc = np.zeros((n,) + terms.shape[1:])
    np.add.at(acc, row, terms)                                         # in entry order
    return acc


# ---- the three calls ----
def sddmm(rowptr, adj, a, b, mean=False):
    """e float32 [E], the sum of |a b| per entry (divided like e for mean) and the unrounded e, float64"""
    _, length, row = _rows(rowptr)
    prod = _f64(a)[row] * _f64(b)[np.asarray(adj, dtype=np.int64)]     # E x F, every product exact in float64
    exact, mag = np.zeros(len(row)), np.zeros(len(row))
    for f in range(prod.shape[1]):                                     # in column order
        exact, mag = exact + prod[:, f], mag + np.abs(prod[:, f])
    if mean:
        exact, mag = exact / length[row], mag / length[row]
    return exact.astype(np.float32), mag, exact


def dot_bound(F):
    """the factor of the sum of |a b|: F products on a chain of F - 1 additions and the division of mean, plus the restatement's own"""
    return AR.tolerance(F)


def edge_softmax(rowptr, e):
    """y float32 [E], the unrounded y, and per entry R = the largest |e - m| over the row's finite entries and d = the row's length"""
    _, length, row = _rows(rowptr)
    e = _f64(e)
    y = softmax64(rowptr, e)
    m = np.full(len(length), -np.inf)
    np.maximum.at(m, row, e)
    R = np.zeros(len(length))
    np.maximum.at(R, row, np.where(np.isfinite(e), m[row] - np.where(np.isfinite(e), e, 0.0), 0.0))
    return y.astype(np.float32), y, R[row], length[row]


def softmax_bound(d, R):
    """relative to the exact y_p, plus TINY absolute: one rounding in e - m moves the exponent by at most R u; one expf error per term, one in the sum,
    one in the hub merge: 3 (R u + eps_exp); at most d - 1 additions of positive terms, the product of the merge, the division: gamma_(d + 3); plus
    the same of the restatement at u = 2^-53 (numpy's exp within an ulp)"""
    d, R = np.asarray(d, dtype=np.float64), np.asarray(R, dtype=np.float64)
    return 3.0 * (R * U32 + EPS_EXP) + gamma(d + 3) + 3.0 * (R * U64 + 2.0 * U64) + gamma(d + 3, U64)


def edge_softmax_backward(rowptr, y, gy):
    """ge float32 [E] = y_p (gy_p - sum_q y_q gy_q) on ANY y, the unrounded ge, and |y_p| (|gy_p| + sum_q |y_q gy_q|)"""
    _, length, row = _rows(rowptr)
    y, gy = _f64(y), _f64(gy)
    exact = softmax_backward64(rowptr, y, gy)
    return exact.astype(np.float32), exact, np.abs(y) * (np.abs(gy) + _row_sum(row, len(length), np.abs(y * gy))[row])


def softmax_backward_bound(d):
    """the factor of |y_p| (|gy_p| + sum |y_q gy_q|): a rounding per product, d - 1 additions, the subtraction, the last product: gamma_(d + 3)"""
    d = np.asarray(d, dtype=np.float64)
    return gamma(d + 3) + gamma(d + 3, U64)


# ---- float64 gradients (no rounding of the weights in between) ----
def spmm64(rowptr, adj, w, x, mean=False):
    """out [n_rows, F] and the sum of |w x|, float64"""
    _, length, row = _rows(rowptr)
    terms = np.asarray(w, dtype=np.float64)[:, None] * np.asarray(x, dtype=np.float64)[np.asarray(adj, dtype=np.int64)]
    out, mag = _row_sum(row, len(length), terms), _row_sum(row, len(length), np.abs(terms))
    if mean:
        scale = np.maximum(length, 1).astype(np.float64)[:, None]
        out, mag = out / scale, mag / scale
    return out, mag


def spmm_backward64(rowptr, adj, n_cols, w, x, g, mean=False):
    """(grad w [E], grad x [n_cols, F]) of sum(out * g), float64"""
    _, length, row = _rows(rowptr)
    adj, g, x, w = np.asarray(adj, dtype=np.int64), np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    coef = 1.0 / length[row] if mean else np.ones(len(row))
    gw = (g[row] * x[adj]).sum(1) * coef
    gx = np.zeros((n_cols, x.shape[1]))
    np.add.at(gx, adj, (w * coef)[:, None] * g[row])
    return gw, gx


def sddmm_backward64(rowptr, adj, n_cols, a, b, ge):
    """(grad a, grad b) of sum(e * ge): the forward run on (b, weight ge) and the transposed run on (a, weight ge)"""
    _, length, row = _rows(rowptr)
    adj, ge = np.asarray(adj, dtype=np.int64), np.asarray(ge, dtype=np.float64)
    ga = _row_sum(row, len(length), ge[:, None] * np.asarray(b, dtype=np.float64)[adj])
    gb = np.zeros((n_cols, np.asarray(a).shape[1]))
    np.add.at(gb, adj, ge[:, None] * np.asarray(a, dtype=np.float64)[row])
    return ga, gb


def softmax64(rowptr, e):
    """the softmax over each row's entries with the -inf rules: exp(-inf) = 0, a row of -inf alone gives 0, -inf - -inf is not formed"""
    _, length, row = _rows(rowptr)
    e, n = np.asarray(e, dtype=np.float64), len(length)
    m = np.full(n, -np.inf)
    np.maximum.at(m, row, e)
    live = m[row] > -np.inf
    with np.errstate(invalid="ignore"):
        t = np.exp(np.where(live, e - np.where(live, m[row], 0.0), -np.inf))
    s = _row_sum(row, n, t)
    return np.where(live, t / np.where(s[row] > 0, s[row], 1.0), 0.0)


def softmax_backward64(rowptr, y, gy):
    _, length, row = _rows(rowptr)
    y, gy = np.asarray(y, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    return y * (gy - _row_sum(row, len(length), y * gy)[row])


def attention(rowptr, adj, q, k, v, scale=None, g=None):
    """dot-product attention of every row over its stored entries, float64: a dict with out [n_rows, Fv], the weights w [E], `bound` (per value of out,
    composed below) and, with a gradient g of out, gq, gk, gv.
    The bound of out computed in float32 from the float32 q, k, v:  the score e_p = scale * dot_p carries eta = scale * dot_bound(F) * sum |q k| + u
    |e_p| (the product with scale); scores off by at most eta move every softmax term and the sum by a factor within exp(+-eta), so w_p is off by
    rel = expm1(2 eta) + exp(2 eta) * (softmax_bound(d, R + 2 eta) + the rounding of w to float32), relative, plus TINY; the weighted sum then adds
    gamma_(d + 2) of the sum of |w v| as any aggregation does:  bound = (rel (1 + tol) + tol) * sum |w_p v_p| + d TINY max |v|."""
    _, length, row = _rows(rowptr)
    adj = np.asarray(adj, dtype=np.int64)
    F = np.asarray(q).shape[1]
    if scale is None:
        scale = float(F) ** -0.5 if F else 1.0
    scale = float(np.float32(scale))
    _, mag, dot = sddmm(rowptr, adj, q, k)
    e = dot * scale
    w = softmax64(rowptr, e)
    out, omag = spmm64(rowptr, adj, w, _f64(v))
    n, d = len(length), int(length.max(initial=0))
    eta_p = scale * dot_bound(F) * mag + U32 * np.abs(e)
    eta = np.zeros(n)
    np.maximum.at(eta, row, eta_p)
    m = np.full(n, -np.inf)
    np.maximum.at(m, row, e)
    R = np.zeros(n)
    np.maximum.at(R, row, m[row] - e)
    rel = np.expm1(2 * eta) + np.exp(2 * eta) * (softmax_bound(length, R + 2 * eta) + U32)
    tol = AR.tolerance(d)
    res = {"out": out, "w": w, "e": e, "bound": (rel * (1 + tol) + tol)[:, None] * omag + length[:, None] * TINY * np.abs(_f64(v)).max(initial=0.0)}
    if g is not None:
        g = np.asarray(g, dtype=np.float64)
        gw, res["gv"] = spmm_backward64(rowptr, adj, np.asarray(k).shape[0], w, _f64(v), g)
        ge = softmax_backward64(rowptr, w, gw) * scale
        res["gq"], res["gk"] = sddmm_backward64(rowptr, adj, np.asarray(k).shape[0], _f64(q), _f64(k), ge)
    return res
