"""The numpy restatement of the edge contract (tests/edge_reference.py) against torch CPU float64 autograd on a row-by-row formulation: torch.softmax
over each row's gathered slice, repeats counted as stored.  Forward and every gradient of sddmm, edge softmax, spmm (both inputs) and attention, the
-inf rules, empty rows, and the values of the bounds at a pinned (d, R, F)."""
import numpy as np
import pytest
import torch

import agg_reference as AR
import edge_reference as ER

LENGTHS = [0, 1, 2, 5, 0, 9, 33, 1, 70, 0, 3]
N_COLS, F = 17, 6


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(1)
    rowptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    adj = rng.integers(0, N_COLS, rowptr[-1]).astype(np.int32)
    adj[rowptr[6]:rowptr[6] + 4] = 3                                   # a repeated entry counts as often as it is stored
    n = len(LENGTHS)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return {"rowptr": rowptr, "adj": adj, "q": f32(n, F), "k": f32(N_COLS, F), "v": f32(N_COLS, 4), "g": f32(n, 4), "ge": f32(len(adj)),
            "e": rng.uniform(-8, 8, len(adj)).astype(np.float32)}


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def row_of(rowptr):
    return torch.repeat_interleave(torch.arange(len(rowptr) - 1), torch.as_tensor(np.diff(rowptr)))


def torch_softmax_rows(rowptr, e):
    """torch.softmax over each row's slice; a row of -inf alone gives 0 by the contract (torch gives NaN there)"""
    parts = []
    for i in range(len(rowptr) - 1):
        s = e[rowptr[i]:rowptr[i + 1]]
        if s.numel():
            parts.append(torch.softmax(s, 0) if bool((s > -np.inf).any()) else torch.zeros_like(s))
    return torch.cat(parts) if parts else e[:0]


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), want.detach().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape, what
    assert np.allclose(got, want, rtol=1e-12, atol=1e-13), (what, float(np.abs(got - want).max(initial=0.0)))


def test_sddmm_forward_and_both_gradients(data):
    rowptr, adj = data["rowptr"], data["adj"]
    a, b = t64(data["q"]), t64(data["k"])
    e = (a[row_of(rowptr)] * b[torch.as_tensor(adj.astype(np.int64))]).sum(-1)
    (e * t64(data["ge"], False)).sum().backward()
    e32, mag, exact = ER.sddmm(rowptr, adj, data["q"], data["k"])
    close(exact, e, "e")
    assert e32.dtype == np.float32 and np.array_equal(e32, exact.astype(np.float32)) and np.all(mag >= np.abs(exact))
    ga, gb = ER.sddmm_backward64(rowptr, adj, N_COLS, data["q"], data["k"], data["ge"])
    close(ga, a.grad, "grad a")
    close(gb, b.grad, "grad b")
    # the same two gradients as the aggregation's restatement states them: the forward and the transposed run with ge as the weight
    close(AR.forward(rowptr, adj, data["k"], "sum", data["ge"], with_abs=True)[3], a.grad, "grad a as a forward run")
    close(AR.backward(rowptr, adj, N_COLS, data["q"], "sum", data["ge"], with_abs=True)[2], b.grad, "grad b as a transposed run")
    _, mag_mean, mean = ER.sddmm(rowptr, adj, data["q"], data["k"], mean=True)
    length = np.diff(rowptr)[row_of(rowptr).numpy()]
    close(mean, exact / length, "mean")
    close(mag_mean, mag / length, "mean magnitudes")


def test_edge_softmax_forward_and_gradient(data):
    rowptr = data["rowptr"]
    e = t64(data["e"])
    y = torch_softmax_rows(rowptr, e)
    (y * t64(data["ge"], False)).sum().backward()
    y32, exact, R, d = ER.edge_softmax(rowptr, data["e"])
    close(exact, y, "y")
    assert y32.dtype == np.float32 and np.array_equal(d, np.diff(rowptr)[row_of(rowptr).numpy()])
    sums = np.zeros(len(LENGTHS))
    np.add.at(sums, row_of(rowptr).numpy(), exact)
    assert np.allclose(sums[np.diff(rowptr) > 0], 1.0, rtol=1e-14)
    e64 = data["e"].astype(np.float64)
    for i in range(len(LENGTHS)):
        lo, hi = rowptr[i], rowptr[i + 1]
        if hi > lo:
            assert np.all(R[lo:hi] == (e64[lo:hi].max() - e64[lo:hi].min()))
    ge32, gexact, gmag = ER.edge_softmax_backward(rowptr, exact.astype(np.float32), data["ge"])
    close(ER.softmax_backward64(rowptr, exact, data["ge"]), e.grad, "grad e")
    assert np.all(gmag >= np.abs(gexact)) and ge32.dtype == np.float32
    # the backward is its formula on any y
    yy = np.abs(data["ge"]) + 1
    _, anyy, _ = ER.edge_softmax_backward(rowptr, yy, data["e"])
    row = row_of(rowptr).numpy()
    dd = np.zeros(len(LENGTHS))
    np.add.at(dd, row, yy.astype(np.float64) * data["e"])
    close(anyy, yy.astype(np.float64) * (data["e"].astype(np.float64) - dd[row]), "any y")


def test_minus_infinity_rules_and_empty_rows():
    inf = np.float32(-np.inf)
    rowptr = np.array([0, 3, 3, 6, 7, 9], dtype=np.int64)
    e = np.array([1.0, inf, 1.0, inf, inf, inf, inf, 2.0, inf], dtype=np.float32)
    y32, exact, R, d = ER.edge_softmax(rowptr, e)
    assert y32.tolist() == [0.5, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0] and not np.isnan(exact).any()
    assert R.tolist() == [0.0] * 9 and d.tolist() == [3, 3, 3, 3, 3, 3, 1, 2, 2]
    close(ER.softmax64(rowptr, e), torch_softmax_rows(rowptr, t64(e, False)), "masked rows")
    empty = np.zeros(4, dtype=np.int64)
    for out in ER.edge_softmax(empty, np.zeros(0, dtype=np.float32)) + ER.edge_softmax_backward(empty, np.zeros(0), np.zeros(0)):
        assert len(out) == 0
    assert len(ER.sddmm(empty, np.zeros(0, dtype=np.int32), np.zeros((3, 2)), np.zeros((5, 2)))[0]) == 0


@pytest.mark.parametrize("mean", [False, True])
def test_spmm_forward_and_both_gradients(data, mean):
    rowptr, adj = data["rowptr"], data["adj"]
    w, x = t64(data["ge"]), t64(data["v"])
    out = torch.zeros((len(LENGTHS), 4), dtype=torch.float64).index_add_(0, row_of(rowptr), w[:, None] * x[torch.as_tensor(adj.astype(np.int64))])
    if mean:
        out = out / torch.as_tensor(np.maximum(np.diff(rowptr), 1)[:, None].astype(np.float64))
    (out * t64(data["g"], False)).sum().backward()
    got, mag = ER.spmm64(rowptr, adj, data["ge"], data["v"], mean)
    close(got, out, "out")
    assert np.all(mag >= np.abs(got))
    gw, gx = ER.spmm_backward64(rowptr, adj, N_COLS, data["ge"], data["v"], data["g"], mean)
    close(gw, w.grad, "grad weight")
    close(gx, x.grad, "grad x")
    close(ER.sddmm(rowptr, adj, data["g"], data["v"], mean)[2], w.grad, "grad weight as sddmm(grad_out, x)")


@pytest.mark.parametrize("scale", [None, 0.25])
def test_attention_forward_and_every_gradient(data, scale):
    rowptr, adj = data["rowptr"], data["adj"]
    q, k, v = t64(data["q"]), t64(data["k"]), t64(data["v"])
    a = torch.as_tensor(adj.astype(np.int64))
    sc = float(np.float32(F ** -0.5 if scale is None else scale))
    w = torch_softmax_rows(rowptr, (q[row_of(rowptr)] * k[a]).sum(-1) * sc)
    out = torch.zeros((len(LENGTHS), 4), dtype=torch.float64).index_add_(0, row_of(rowptr), w[:, None] * v[a])
    (out * t64(data["g"], False)).sum().backward()
    r = ER.attention(rowptr, adj, data["q"], data["k"], data["v"], scale, data["g"])
    for name, want in (("out", out), ("w", w), ("gq", q.grad), ("gk", k.grad), ("gv", v.grad)):
        close(r[name], want, name)
    assert r["bound"].shape == (len(LENGTHS), 4) and np.all(r["bound"] >= 0) and not r["bound"][0].any()        # an empty row: 0 within 0
    assert np.all(r["bound"][np.diff(rowptr) > 0] < 1e-4 * np.abs(data["v"]).max())


def test_the_bounds_at_a_pinned_point():
    u, v = 2.0 ** -24, 2.0 ** -53
    assert ER.EXP_ULPS == ER.EXP_ULPS_MEASURED + 1 and ER.EPS_EXP == ER.EXP_ULPS * 2.0 ** -23
    g32, g64 = 103 * u / (1 - 103 * u), 103 * v / (1 - 103 * v)
    assert ER.softmax_bound(100, 16.0) == pytest.approx(3 * (16 * u + ER.EPS_EXP) + g32 + 3 * (16 * v + 2 * v) + g64, rel=1e-15)
    assert ER.softmax_backward_bound(100) == pytest.approx(g32 + g64, rel=1e-15)
    assert ER.dot_bound(64) == AR.tolerance(64) == pytest.approx(66 * u / (1 - 66 * u) + 66 * v / (1 - 66 * v), rel=1e-15)
    assert ER.gamma(5) == pytest.approx(5 * u / (1 - 5 * u), rel=1e-15) and ER.TINY == 2.0 ** -126
