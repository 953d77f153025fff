"""The numpy restatement of the GAT contract (tests/gat_reference.py) against torch CPU: the float32 score bit for bit against
F.leaky_relu(s[row] + t[adj], slope), the sums and every gradient against float64 autograd of the whole GAT formulation, on a CSR with empty rows,
repeated entries and self entries; slope 1, 0.2 and 0, an absent term, the E x H layout, the bound of the sums and the bytes model.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import agg_reference as AR
import gat_reference as GR

SLOPES = [1.0, 0.2, 0.0]


def small_csr():
    """7 rows over 7 columns: two empty rows, a row that lists itself twice, a row that lists one neighbour three times; column 3 is never listed
    but once"""
    rows = [[0, 0, 3], [], [1, 1, 1, 2, 5], [6], [], [4, 4, 0, 2, 2, 6, 1], [5]]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.array([v for r in rows for v in r], dtype=np.int32), 7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", [1, 2, 3, 8])
def test_score_is_torch_leaky_relu_bit_for_bit(H, slope):
    rng = np.random.default_rng(10 + H)
    rowptr, adj, n_cols = small_csr()
    n, E = len(rowptr) - 1, len(adj)
    s, t = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((n_cols, H)).astype(np.float32)
    s[0, 0], t[0, 0], t[3, 0] = 0.0, -0.0, -0.0                         # signed zeros: 0 + -0 = 0, and a -0 that is scaled
    row, a = torch.as_tensor(GR.row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    want = F.leaky_relu(torch.tensor(s)[row] + torch.tensor(t)[a], slope).numpy()
    got = GR.score(rowptr, adj, s, t, slope)
    assert got.shape == (E, H) and got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    if slope == 1.0:                                                   # the identity on bits
        assert np.array_equal(bits(got), bits(s[GR.row_index(rowptr)] + t[adj]))


def test_score_layout_and_one_dimensional_terms():
    rng = np.random.default_rng(2)
    rowptr, adj, n_cols = small_csr()
    s, t = rng.standard_normal((7, 3)).astype(np.float32), rng.standard_normal((n_cols, 3)).astype(np.float32)
    e = GR.score(rowptr, adj, s, t, 0.2)
    row = GR.row_index(rowptr)
    for p in range(len(adj)):
        for h in range(3):                                             # e[p * H + h]
            z = np.float32(s[row[p], h] + t[adj[p], h])
            assert e.reshape(-1)[p * 3 + h] == (z if z > 0 else np.float32(0.2) * z)
    for h in range(3):
        assert np.array_equal(bits(GR.score(rowptr, adj, s[:, h], t[:, h], 0.2)[:, 0]), bits(e[:, h]))


@pytest.mark.parametrize("slope", SLOPES)
def test_an_absent_term_is_a_broadcast_with_its_bits(slope):
    rng = np.random.default_rng(3)
    rowptr, adj, n_cols = small_csr()
    s, t = rng.standard_normal((7, 2)).astype(np.float32), rng.standard_normal((n_cols, 2)).astype(np.float32)
    s[2, 1], t[1, 0] = -0.0, -0.0
    row = GR.row_index(rowptr)
    for got, z in ((GR.score(rowptr, adj, s, None, slope), s[row]), (GR.score(rowptr, adj, None, t, slope), t[adj])):
        want = F.leaky_relu(torch.tensor(z), slope).numpy()
        assert np.array_equal(bits(got), bits(want))
    # nothing is added: with slope 1 a -0 stays -0, which 0 + -0 would not
    assert np.array_equal(bits(GR.score(rowptr, adj, s, None, 1.0)), bits(s[row])) and np.signbit(GR.score(rowptr, adj, s, None, 1.0)[row == 2][:, 1]).all()
    assert np.array_equal(bits(GR.score(rowptr, adj, None, t, 1.0)), bits(t[adj]))


def torch_gat(rowptr, adj, s, t, v, slope):
    """the whole formulation on torch float64 leaves: (e, w, out), e and w of shape E x H"""
    n, H = s.shape
    Dv = v.shape[1] // H
    row, a = torch.as_tensor(GR.row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    e = F.leaky_relu(s[row] + t[a], slope)
    w = torch.cat([torch.softmax(e[rowptr[i]:rowptr[i + 1]], 0) for i in range(n)])
    out = torch.zeros((n, H, Dv), dtype=torch.float64).index_add_(0, row, w[:, :, None] * v[a].view(-1, H, Dv))
    return e, w, out.view(n, H * Dv)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", [1, 2, 4, 3])
def test_restatement_equals_torch_autograd_of_the_whole_formulation(H, slope):
    rng = np.random.default_rng(40 + H)
    rowptr, adj, n_cols = small_csr()
    n, E = len(rowptr) - 1, len(adj)
    s, t, v, g = (rng.standard_normal(shape) for shape in ((n, H), (n_cols, H), (n_cols, 3 * H), (n, 3 * H)))
    s, t, v, g = (x.astype(np.float32).astype(np.float64) for x in (s, t, v, g))
    st, tt, vt = (torch.tensor(x, requires_grad=True) for x in (s, t, v))
    e, w, out = torch_gat(rowptr, adj, st, tt, vt, slope)
    (out * torch.as_tensor(g)).sum().backward()
    r = GR.attention(rowptr, adj, s, t, v, slope, g=g)
    assert r["w"].shape == (E, H) and r["out"].shape == (n, 3 * H) and (r["bound"] >= 0).all()
    for got, want, what in ((r["e"], e.detach().numpy(), "e"), (r["w"], w.detach().numpy(), "w"), (r["out"], out.detach().numpy(), "out"),
                            (r["gs"], st.grad.numpy(), "gs"), (r["gt"], tt.grad.numpy(), "gt"), (r["gv"], vt.grad.numpy(), "gv")):
        assert np.allclose(got, want, rtol=1e-12, atol=1e-13), what
    assert not r["out"][[1, 4]].any() and not r["gs"][[1, 4]].any()     # the empty rows


@pytest.mark.parametrize("slope", SLOPES)
def test_score_gradients_are_the_two_gated_sums(slope):
    """grad s and grad t of sum(e * ge) from torch autograd ARE edge_sum(ge, gate = e) forward and transposed: the saved score is the gate"""
    rng = np.random.default_rng(5)
    rowptr, adj, n_cols = small_csr()
    H = 3
    s, t = rng.standard_normal((7, H)).astype(np.float32), rng.standard_normal((n_cols, H)).astype(np.float32)
    ge = rng.integers(-8, 9, (len(adj), H)).astype(np.float32)
    st, tt = torch.tensor(s, dtype=torch.float64, requires_grad=True), torch.tensor(t, dtype=torch.float64, requires_grad=True)
    row, a = torch.as_tensor(GR.row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    (F.leaky_relu(st[row] + tt[a], slope) * torch.tensor(ge, dtype=torch.float64)).sum().backward()
    e = GR.score(rowptr, adj, s, t, slope)
    gs, mag_s, exact_s, d_s = GR.edge_sum(rowptr, adj, n_cols, ge, gate=e, slope=slope)
    gt, mag_t, exact_t, d_t = GR.edge_sum(rowptr, adj, n_cols, ge, gate=e, slope=slope, transposed=True)
    slope32 = float(np.float32(slope))                                 # the sums take the slope as a float32
    want_s, want_t = GR.score_backward64(rowptr, adj, n_cols, e, ge, slope32)
    assert np.allclose(want_s, st.grad.numpy(), rtol=1e-7, atol=1e-7) and np.allclose(want_t, tt.grad.numpy(), rtol=1e-7, atol=1e-7)
    assert np.allclose(exact_s, want_s, rtol=1e-14, atol=1e-14) and np.allclose(exact_t, want_t, rtol=1e-14, atol=1e-14)
    assert np.array_equal(d_s, np.diff(rowptr)) and np.array_equal(d_t, np.bincount(adj, minlength=n_cols))
    assert (mag_s >= np.abs(exact_s) - 1e-12).all() and (np.abs(gs - exact_s) <= GR.sum_bound(d_s)[:, None] * mag_s).all()
    assert (np.abs(gt - exact_t) <= GR.sum_bound(d_t)[:, None] * mag_t).all()
    assert not gs[[1, 4]].any() and gs.shape == (7, H) and gt.shape == (n_cols, H)


def test_sum_gradient_is_the_broadcast():
    """the gradient of edge_sum with respect to w is the score with one term absent and slope 1: the pair closes under differentiation"""
    rng = np.random.default_rng(6)
    rowptr, adj, n_cols = small_csr()
    w = rng.standard_normal((len(adj), 2))
    row, a = torch.as_tensor(GR.row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    for transposed, index, n in ((False, row, 7), (True, a, n_cols)):
        g = rng.standard_normal((n, 2)).astype(np.float32)
        wt = torch.tensor(w, requires_grad=True)
        out = torch.zeros((n, 2), dtype=torch.float64).index_add_(0, index, wt)
        (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
        assert np.allclose(GR.edge_sum(rowptr, adj, n_cols, w.astype(np.float32), transposed=transposed)[2], out.detach().numpy(), rtol=1e-6, atol=1e-6)
        got = GR.score(rowptr, adj, None, g, 1.0) if transposed else GR.score(rowptr, adj, g, None, 1.0)
        assert np.array_equal(got, wt.grad.numpy().astype(np.float32))


def test_gate_sign_per_head_and_gated_exactness_on_integers():
    rowptr, adj, n_cols = small_csr()
    E = len(adj)
    w = np.arange(E * 2, dtype=np.float32).reshape(E, 2) - 8
    gate = np.stack([np.ones(E), -np.ones(E)], axis=1).astype(np.float32)       # head 0 open, head 1 gated
    out, mag, exact, _ = GR.edge_sum(rowptr, adj, n_cols, w, gate=gate, slope=0.25)
    plain = GR.edge_sum(rowptr, adj, n_cols, w)[2]
    assert np.array_equal(exact[:, 0], plain[:, 0]) and np.array_equal(exact[:, 1], 0.25 * plain[:, 1]) and np.array_equal(out, exact.astype(np.float32))
    zero = GR.edge_sum(rowptr, adj, n_cols, w, gate=np.zeros((E, 2), dtype=np.float32), slope=0.25)[2]      # a gate at 0 takes the slope, as torch does
    assert np.array_equal(zero, 0.25 * plain)


def test_bytes_model_terms():
    rowptr = np.array([0, 3, 3, 40, 40 + 2000], dtype=np.int64)        # short, empty, wave, workgroup (one chunk)
    c = AR.classify(rowptr)
    assert (c["rows_short"], c["rows_wave"], c["rows_wg"], c["chunks"]) == (2, 1, 1, 1)
    E, H, lists = 2040, 4, 4 * 3 + 8
    assert GR.bytes_score(rowptr, H) == E * (4 + 16 + 16) + 4 * (8 + 16) + lists
    assert GR.bytes_score(rowptr, H, has_s=False) == E * (4 + 16 + 16) + 4 * 8 + lists
    assert GR.bytes_score(rowptr, H, has_t=False) == E * (4 + 16) + 4 * (8 + 16) + lists
    assert GR.bytes_sum(rowptr, H) == E * 16 + 4 * (8 + 16) + lists
    assert GR.bytes_sum(rowptr, H, gate=True) == E * 32 + 4 * (8 + 16) + lists
    assert GR.bytes_sum(rowptr, H, gate=True, transposed=True) == E * 36 + 4 * (8 + 16) + lists
    assert [GR.vec_of(h) for h in (1, 2, 3, 4, 5, 8, 12, 16, 64)] == [1, 1, 1, 4, 1, 4, 4, 4, 4] and GR.vec_of(8, wide=False) == 1
