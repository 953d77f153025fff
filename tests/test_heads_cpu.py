"""The numpy restatement of the heads contract (tests/heads_reference.py) against torch CPU float64 autograd on a per-head formulation, on a CSR with
empty rows, repeated entries and self entries; the -inf rules per head, the E x H layout, H = 1 equal to the single-head restatement, and the
bytes model.  No GPU."""
import numpy as np
import pytest
import torch

import agg_reference as AR
import edge_reference as ER
import heads_reference as HR


def small_csr():
    """7 rows over 7 columns: two empty rows, a row that lists itself twice, a row that lists one neighbour three times"""
    rows = [[0, 0, 3], [], [1, 1, 1, 2, 5], [6], [], [4, 4, 0, 2, 2, 6, 1], [5]]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.array([v for r in rows for v in r], dtype=np.int32), 7


def row_index(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def torch_attention(rowptr, adj, q, k, v, H, scale, op="sum"):
    """per-head formulation on torch float64 leaves: returns (e, w, out) with e, w of shape E x H"""
    n, F = q.shape
    D, Dv = F // H, v.shape[1] // H
    row, a = torch.as_tensor(row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    e = (q[row].view(-1, H, D) * k[a].view(-1, H, D)).sum(-1)
    w = torch.cat([torch.softmax(e[rowptr[i]:rowptr[i + 1]] * scale, 0) for i in range(n)])
    out = torch.zeros((n, H, Dv), dtype=torch.float64).index_add_(0, row, w[:, :, None] * v[a].view(-1, H, Dv))
    return e, w, out.view(n, H * Dv)


@pytest.mark.parametrize("H,D", [(1, 4), (2, 3), (4, 2), (3, 1)])
def test_restatement_equals_torch_autograd_per_head(H, D):
    rng = np.random.default_rng(40 + H)
    rowptr, adj, n_cols = small_csr()
    n, F, E = len(rowptr) - 1, H * D, len(adj)
    q, k, v, g = (rng.standard_normal(s) * 0.5 for s in ((n, F), (n_cols, F), (n_cols, 2 * H), (n, 2 * H)))
    q, k, v, g = (t.astype(np.float32).astype(np.float64) for t in (q, k, v, g))
    qt, kt, vt = (torch.tensor(t, requires_grad=True) for t in (q, k, v))
    scale = float(np.float32(D ** -0.5))
    e, w, out = torch_attention(rowptr, adj, qt, kt, vt, H, scale)
    (out * torch.as_tensor(g)).sum().backward()
    r = HR.attention(rowptr, adj, q, k, v, H, g=g)
    assert r["w"].shape == (E, H) and r["out"].shape == (n, 2 * H)
    for got, want, what in ((r["e"], e.detach().numpy() * scale, "e"), (r["w"], w.detach().numpy(), "w"), (r["out"], out.detach().numpy(), "out"),
                            (r["gq"], qt.grad.numpy(), "gq"), (r["gk"], kt.grad.numpy(), "gk"), (r["gv"], vt.grad.numpy(), "gv")):
        assert np.allclose(got, want, rtol=1e-12, atol=1e-13), what
    # the five calls, each against the same formulation
    e32, mag, exact = HR.sddmm(rowptr, adj, q, k, H)
    assert e32.shape == (E, H) and np.allclose(exact, e.detach().numpy(), rtol=1e-12, atol=1e-13) and (mag >= np.abs(exact) - 1e-12).all()
    wts = rng.integers(-3, 4, (E, H)).astype(np.float64)
    for op in ("sum", "mean"):
        wt, xt = torch.tensor(wts, requires_grad=True), torch.tensor(v, requires_grad=True)
        row, a = torch.as_tensor(row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
        ref = torch.zeros((n, H, 2), dtype=torch.float64).index_add_(0, row, wt[:, :, None] * xt[a].view(-1, H, 2)).view(n, 2 * H)
        if op == "mean":
            ref = ref / torch.as_tensor(np.maximum(np.diff(rowptr), 1)[:, None].astype(np.float64))
        (ref * torch.as_tensor(g)).sum().backward()
        out32, omag, oexact = HR.run(rowptr, adj, v, op, wts)
        assert np.allclose(oexact, ref.detach().numpy(), rtol=1e-12, atol=1e-13), op
        gw, gx = HR.spmm_backward64(rowptr, adj, n_cols, wts, v, g, mean=op == "mean")
        assert np.allclose(gw, wt.grad.numpy(), rtol=1e-12, atol=1e-13) and np.allclose(gx, xt.grad.numpy(), rtol=1e-12, atol=1e-13), op
        # the transposed run IS grad x, and the heads dot product of (g, x) IS grad w
        assert np.allclose(HR.run_transposed(rowptr, adj, n_cols, g, op, wts)[2], gx, rtol=1e-12, atol=1e-13), op
        assert np.allclose(HR.sddmm(rowptr, adj, g, v, H, mean=op == "mean")[2], gw, rtol=1e-12, atol=1e-13), op
    ge = rng.integers(-3, 4, (E, H)).astype(np.float64)
    qt, kt = torch.tensor(q, requires_grad=True), torch.tensor(k, requires_grad=True)
    (torch_attention(rowptr, adj, qt, kt, vt.detach(), H, scale)[0] * torch.as_tensor(ge)).sum().backward()
    ga, gb = HR.sddmm_backward64(rowptr, adj, n_cols, q, k, ge, H)
    assert np.allclose(ga, qt.grad.numpy(), rtol=1e-12, atol=1e-13) and np.allclose(gb, kt.grad.numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(ga, HR.run(rowptr, adj, k, "sum", ge)[2]) and np.allclose(gb, HR.run_transposed(rowptr, adj, n_cols, q, "sum", ge)[2])
    # the softmax and its backward per column
    e32 = r["e"].astype(np.float32)                                    # the call takes float32 scores
    et = torch.tensor(e32.astype(np.float64), requires_grad=True)
    y = torch.cat([torch.softmax(et[rowptr[i]:rowptr[i + 1]], 0) for i in range(n)])
    (y * torch.as_tensor(ge)).sum().backward()
    assert np.allclose(HR.edge_softmax(rowptr, e32)[1], y.detach().numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(HR.softmax_backward64(rowptr, y.detach().numpy(), ge), et.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_minus_infinity_rules_hold_per_head():
    rowptr, adj, _ = small_csr()
    E = len(adj)
    e = np.zeros((E, 3), dtype=np.float32)
    e[:, 1] = -np.inf                                                  # head 1: every row dead
    e[rowptr[5]:rowptr[5] + 3, 0] = -np.inf                            # head 0: three entries of row 5 dead
    e[rowptr[2]:rowptr[3], 2] = -np.inf                                # head 2: row 2 dead
    y, exact, R, d = HR.edge_softmax(rowptr, e)
    assert y.shape == (E, 3) and not np.isnan(y).any() and not y[:, 1].any()
    row5 = y[rowptr[5]:rowptr[6]]
    assert not row5[:3, 0].any() and np.array_equal(row5[3:, 0], np.full(4, np.float32(0.25))) and np.array_equal(row5[:, 2], np.full(7, np.float32(1) / np.float32(7)))
    assert not y[rowptr[2]:rowptr[3], 2].any() and np.array_equal(y[rowptr[2]:rowptr[3], 0], np.full(5, np.float32(0.2)))
    assert np.array_equal(d[:, 0], np.diff(rowptr)[row_index(rowptr)])


def test_layout_is_entries_by_heads_and_a_head_is_its_column_slice():
    rng = np.random.default_rng(41)
    rowptr, adj, n_cols = small_csr()
    H, D, E = 3, 2, len(adj)
    a, b = rng.integers(-8, 9, (len(rowptr) - 1, H * D)).astype(np.float32), rng.integers(-8, 9, (n_cols, H * D)).astype(np.float32)
    e = HR.sddmm(rowptr, adj, a, b, H)[0]
    assert e.shape == (E, H) and e.flags["C_CONTIGUOUS"]
    row = row_index(rowptr)
    for p in (0, 4, E - 1):
        for h in range(H):
            assert e[p, h] == np.dot(a[row[p], h * D:(h + 1) * D], b[adj[p], h * D:(h + 1) * D]) == e.ravel()[p * H + h]
    w = rng.integers(-8, 9, (E, H)).astype(np.float32)
    out = HR.run(rowptr, adj, b, "sum", w)[0]
    for h in range(H):
        assert np.array_equal(out[:, h * D:(h + 1) * D], AR.forward(rowptr, adj, b[:, h * D:(h + 1) * D], "sum", w[:, h])[0])
    same = np.repeat(w[:, :1], H, axis=1)                              # equal weight columns: the single-head call of the whole width
    assert np.array_equal(HR.run(rowptr, adj, b, "mean", same)[0], AR.forward(rowptr, adj, b, "mean", w[:, 0])[0])
    assert np.array_equal(HR.run_transposed(rowptr, adj, n_cols, a, "mean", same)[0], AR.backward(rowptr, adj, n_cols, a, "mean", w[:, 0]))


def test_one_head_is_the_single_head_restatement():
    rng = np.random.default_rng(42)
    rowptr, adj, n_cols = small_csr()
    n, E, F = len(rowptr) - 1, len(adj), 5
    a, b, g = (rng.standard_normal(s).astype(np.float32) for s in ((n, F), (n_cols, F), (n, F)))
    e, gy = rng.uniform(-8, 8, E).astype(np.float32), rng.standard_normal(E).astype(np.float32)
    for mean in (False, True):
        for got, want in zip(HR.sddmm(rowptr, adj, a, b, 1, mean=mean), ER.sddmm(rowptr, adj, a, b, mean=mean)):
            assert np.array_equal(got[:, 0], want)
    for got, want in zip(HR.edge_softmax(rowptr, e[:, None]), ER.edge_softmax(rowptr, e)):
        assert np.array_equal(got[:, 0], want)
    y = ER.edge_softmax(rowptr, e)[0]
    for got, want in zip(HR.edge_softmax_backward(rowptr, y[:, None], gy[:, None]), ER.edge_softmax_backward(rowptr, y, gy)):
        assert np.array_equal(got[:, 0], want)
    for op in ("sum", "mean"):
        want = AR.forward(rowptr, adj, b, op, e, with_abs=True)
        assert all(np.array_equal(p, r) for p, r in zip(HR.run(rowptr, adj, b, op, e[:, None]), (want[0], want[2], want[3])))
        assert all(np.array_equal(p, r) for p, r in zip(HR.run_transposed(rowptr, adj, n_cols, g, op, e[:, None]), AR.backward(rowptr, adj, n_cols, g, op, e, with_abs=True)))
    r1, r = HR.attention(rowptr, adj, a, b, b, 1, g=g), ER.attention(rowptr, adj, a, b, b, g=g)
    assert all(np.array_equal(r1[key], r[key]) for key in ("out", "bound", "gq", "gk", "gv")) and np.array_equal(r1["w"][:, 0], r["w"])


def test_bytes_model_and_walks():
    rowptr = np.array([0, 2, 2, 5], dtype=np.int64)
    assert HR.dot_walks(4, 1, 4) == [1, 1, 1] == AR.column_tiles(4, 4) and HR.dot_walks(260, 1, 4) == AR.column_tiles(260, 4) == [9, 2, 2]
    assert HR.dot_walks(64, 4, 4) == [2, 1, 1]                         # 4 lanes per head: two heads beside each other in a short team, all four in a wave
    assert HR.dot_walks(64, 64, 1) == [8, 1, 1] and HR.dot_walks(72, 2, 4) == [4, 1, 1] and HR.dot_walks(520, 2, 4) == [18, 4, 4]
    assert HR.dot_walks(9, 3, 1) == [2, 1, 1] and HR.dot_walks(36, 3, 4) == [2, 1, 1]
    assert HR.class_entries(rowptr) == [5, 0, 0]
    # with one head the models are those of the single-head calls (tests/test_edge_gpu.py has the same figures)
    assert HR.bytes_sddmm(rowptr, 4, 1, 4) == 5 * 4 + 5 * (4 * 4 + 4) + 3 * (8 + 4 * 4) + 3 * 4
    assert HR.bytes_softmax(rowptr, 1) == 5 * (4 * 3 + 4) + 3 * 8 + 3 * 4 and HR.bytes_softmax(rowptr, 1, backward=True) == 5 * (8 * 2 + 4) + 3 * 8 + 3 * 4
    assert HR.bytes_sddmm(rowptr, 8, 2, 4) == 5 * 4 + 5 * (4 * 8 + 4 * 2) + 3 * (8 + 4 * 8) + 3 * 4
    assert HR.bytes_softmax(rowptr, 4) == 5 * 4 * 16 + 3 * 8 + 3 * 4
    assert HR.bytes_run(rowptr, 8, 2, 4) == 5 * (4 + 8) + 5 * 32 + 3 * (8 + 32) + 3 * 4
    assert HR.bytes_run(rowptr, 8, 2, 4, transposed=True, mean=True) == 5 * (4 + 8 + 4 + 16) + 5 * 32 + 3 * (8 + 32) + 3 * 4
