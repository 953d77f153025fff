"""CPU tests that pin the numpy restatement of the aggregation contract (tests/agg_reference.py) against scipy's sparse product, torch CPU autograd on
the dense formulation, and hand-made cases: the tie rule of the arg, empty rows, the order inside the transpose, the row classes, the tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import agg_reference as R  # noqa: E402


def random_csr(rng, n_rows, n_cols, max_len, empty_every=5):
    length = rng.integers(0, max_len + 1, n_rows)
    length[::empty_every] = 0
    rowptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    adj = rng.integers(0, n_cols, rowptr[-1]).astype(np.int32)         # repeats and self entries happen
    return rowptr, adj


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(29)
    rowptr, adj = random_csr(rng, 40, 23, 9)
    x = rng.standard_normal((23, 5)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, len(adj)).astype(np.float32)
    g = rng.standard_normal((40, 5)).astype(np.float32)
    return rowptr, adj, x, w, g


def test_sum_matches_scipy(case):
    import scipy.sparse as sp
    rowptr, adj, x, w, _ = case
    for weight in (None, w):
        data = np.ones(len(adj)) if weight is None else weight.astype(np.float64)
        ref = sp.csr_matrix((data, adj, rowptr), shape=(40, 23)) @ x.astype(np.float64)      # duplicates are summed
        out, arg, mag, exact = R.forward(rowptr, adj, x, "sum", weight, with_abs=True)
        assert arg is None
        assert np.all(np.abs(exact - ref) <= R.tolerance(9) * mag + 1e-300)
        assert np.array_equal(out, exact.astype(np.float32))
        length = np.maximum(np.diff(rowptr), 1)[:, None]
        mean, _ = R.forward(rowptr, adj, x, "mean", weight)
        assert np.allclose(mean, ref / length, rtol=1e-6, atol=1e-7)


def dense_forward(rowptr, adj, x, op, w):
    """torch CPU, float64, the dense formulation: repeated entries are counted"""
    n_rows, E = len(rowptr) - 1, len(adj)
    row = torch.repeat_interleave(torch.arange(n_rows), torch.as_tensor(np.diff(rowptr)))
    a = torch.as_tensor(adj.astype(np.int64))
    if op in ("sum", "mean"):
        A = torch.zeros((n_rows, x.shape[0]), dtype=torch.float64)
        A.index_put_((row, a), torch.ones(E, dtype=torch.float64) if w is None else torch.as_tensor(w.astype(np.float64)), accumulate=True)
        out = A @ x
        return out / torch.as_tensor(np.maximum(np.diff(rowptr), 1)[:, None].astype(np.float64)) if op == "mean" else out
    rows = []
    for i in range(n_rows):
        seg = x[a[rowptr[i]:rowptr[i + 1]]]
        if seg.shape[0] == 0:
            rows.append(torch.zeros(x.shape[1], dtype=torch.float64))
        else:
            rows.append(seg.max(0).values if op == "max" else seg.min(0).values)
    return torch.stack(rows)


@pytest.mark.parametrize("op,weighted", [("sum", False), ("sum", True), ("mean", False), ("mean", True), ("max", False), ("min", False)])
def test_forward_and_gradient_match_torch_cpu_autograd(case, op, weighted):
    rowptr, adj, x, w, g = case
    weight = w if weighted else None
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    ref = dense_forward(rowptr, adj, xt, op, weight)
    ref.backward(torch.as_tensor(g.astype(np.float64)))
    out, arg, mag, _ = R.forward(rowptr, adj, x, op, weight, with_abs=True)
    assert np.all(np.abs(out - ref.detach().numpy()) <= R.tolerance(9) * mag + 1e-300)
    gx, gmag, _ = R.backward(rowptr, adj, 23, g, op, weight, arg, with_abs=True)
    assert np.all(np.abs(gx - xt.grad.numpy()) <= R.tolerance(40 * 9) * gmag + 1e-300)   # (real-valued data: no ties for max / min)


def test_arg_takes_the_smallest_position_on_ties():
    rowptr = np.array([0, 4, 4, 7], dtype=np.int64)
    adj = np.array([2, 0, 2, 1, 1, 1, 0], dtype=np.int32)
    x = np.array([[1.0, 5.0], [3.0, 5.0], [3.0, 5.0]], dtype=np.float32)
    out, arg = R.forward(rowptr, adj, x, "max")
    assert out.tolist() == [[3.0, 5.0], [0.0, 0.0], [3.0, 5.0]]
    assert arg.tolist() == [[0, 0], [-1, -1], [4, 4]]
    out, arg = R.forward(rowptr, adj, x, "min")
    assert out.tolist() == [[1.0, 5.0], [0.0, 0.0], [1.0, 5.0]]
    assert arg.tolist() == [[1, 0], [-1, -1], [6, 4]]
    g = np.ones((3, 2), dtype=np.float32)
    gx = R.backward(rowptr, adj, 3, g, "max", arg=R.forward(rowptr, adj, x, "max")[1])
    assert gx.tolist() == [[0.0, 0.0], [1.0, 1.0], [1.0, 1.0]]         # position 0 reads column 2, position 4 column 1


def test_empty_rows_and_empty_csr():
    rowptr = np.array([0, 0, 2, 2], dtype=np.int64)
    adj = np.array([1, 1], dtype=np.int32)
    x = np.array([[7.0], [2.0]], dtype=np.float32)
    for op, want in (("sum", 4.0), ("mean", 2.0), ("max", 2.0), ("min", 2.0)):
        out, arg = R.forward(rowptr, adj, x, op)
        assert out[:, 0].tolist() == [0.0, want, 0.0]
        if arg is not None:
            assert arg[:, 0].tolist() == [-1, 0, -1]
    out, arg = R.forward(np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32), x, "max")
    assert out.tolist() == [[0.0], [0.0]] and arg.tolist() == [[-1], [-1]]
    assert R.backward(np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32), 2, np.ones((2, 1), dtype=np.float32), "sum").tolist() == [[0.0], [0.0]]


def test_transpose_is_ascending_in_position_within_every_row(case):
    rowptr, adj, _, _, _ = case
    t_rowptr, t_row, origin = R.transpose(rowptr, adj, 23)
    assert t_rowptr[0] == 0 and t_rowptr[-1] == len(adj) and sorted(origin.tolist()) == list(range(len(adj)))
    row = np.repeat(np.arange(40), np.diff(rowptr))
    for u in range(23):
        seg = origin[t_rowptr[u]:t_rowptr[u + 1]]
        assert (adj[seg] == u).all() and (np.diff(seg) > 0).all()
        assert (t_row[t_rowptr[u]:t_rowptr[u + 1]] == row[seg]).all()


def test_classification_and_chunk_counts_are_pinned():
    length = [0, 1, 32, 33, 1024, 1025, 16384, 16385, 40000, 0]
    rowptr = np.concatenate([[0], np.cumsum(length)])
    assert R.classify(rowptr) == {"rows": 10, "entries": sum(length), "rows_short": 4, "rows_wave": 2, "rows_wg": 4, "chunks": 1 + 1 + 2 + 3, "hub_rows": 2}
    assert R.classify(rowptr, short=4, wave=16, chunk=64) == {"rows": 10, "entries": sum(length), "rows_short": 3, "rows_wave": 0, "rows_wg": 7,
                                                                "chunks": 1 + 1 + 16 + 17 + 256 + 257 + 625, "hub_rows": 5}
    assert R.chunks_of(40000, 16) == 16 and R.chunks_of(32768 * 16 + 1, 16) == 17
    assert R.column_tiles(64, 4) == [2, 1, 1] and R.column_tiles(3, 1) == [1, 1, 1] and R.column_tiles(260, 4) == [9, 2, 2] and R.column_tiles(65, 1) == [9, 2, 2]


def test_tolerance_is_pinned():
    assert R.tolerance(10) == 7.152562502280908e-07
    assert R.tolerance(10) == 12 * 2.0 ** -24 / (1 - 12 * 2.0 ** -24) + 12 * 2.0 ** -53 / (1 - 12 * 2.0 ** -53)
    assert R.tolerance(0) < R.tolerance(1) < R.tolerance(1000)
