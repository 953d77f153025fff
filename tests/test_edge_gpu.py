"""Edge scores, edge softmax and graph attention on the GPU (vgl_hip_agg_sddmm / _edge_softmax / _edge_softmax_backward, api.sddmm / edge_softmax /
spmm / graph_attention, apps/bin/attn_hip) against the numpy restatement of the contract (tests/edge_reference.py).  As in test_agg_gpu.py most
comparisons are on data where every product and partial sum is exact in float32, so results are compared for EQUALITY: integer features for the dot
products, scores constant per row (exp(0) = 1, one division) and masks at -inf for the softmax, y in {0.25, 0.5, 1} with integer gradients for its
backward, q = 0 on rows of power-of-two length for attention.  Real-valued data is held to the derived bounds, with |e| <= 8 so that the largest
|e - m| stays inside the expf sweep of DESIGN section 30."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import agg_reference as AR
import edge_reference as ER

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHRUNK = {"VGL_AGG_SHORT": "4", "VGL_AGG_WAVE": "16", "VGL_AGG_CHUNK": "64"}
LONG = list(range(67)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
NEG_INF = np.float32(-np.inf)


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def lib():
    from vectorgraphlibrary_amd import lib as L
    return L


def csr_of(lengths, n_cols, rng):
    lengths = np.asarray(lengths, dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rowptr, rng.integers(0, n_cols, rowptr[-1]).astype(np.int32)


def ints(rng, *shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


def dev(ctx, a):
    return torch.tensor(a, device=ctx.device)


def host(t):
    return t.detach().cpu().numpy()


def plan_of(ctx, rowptr, adj, n_cols):
    return api().AggregationPlan(ctx, dev(ctx, rowptr), dev(ctx, adj), n_cols)


def shrink(monkeypatch):
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    return {"short": 4, "wave": 16, "chunk": 64}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def row_index(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def check_stats(plan, rowptr, F, vec, **switches):
    st = plan.last_edge_stats
    for k, v in AR.classify(rowptr, **switches).items():
        assert st[k] == v and plan.info()[k] == v, (k, st[k], v)
    assert st["column_tiles"] == (AR.column_tiles(F, vec) if F else [1, 1, 1]) and st["vec"] == vec and st["transposed"] == 0
    assert st["algorithmic_bytes"] > 4 * st["entries"] * max(F, 1)


# ---- SDDMM on integer data, compared for equality ----
def check_dot(ctx, plan, rowptr, adj, n_cols, F, rng, what, vec=None, **switches):
    A = api()
    a, b = ints(rng, len(rowptr) - 1, F), ints(rng, n_cols, F)
    e = A.sddmm(plan, dev(ctx, a), dev(ctx, b))
    assert e.dtype == torch.float32 and tuple(e.shape) == (len(adj),), what
    assert np.array_equal(host(e), ER.sddmm(rowptr, adj, a, b)[0]), what
    check_stats(plan, rowptr, F, (4 if F % 4 == 0 else 1) if vec is None else vec, **switches)
    mean = plan._sddmm(dev(ctx, a), dev(ctx, b), 1)                     # an exact sum, one correctly rounded division
    assert np.array_equal(host(mean), ER.sddmm(rowptr, adj, a, b, mean=True)[0]), what + " mean"


@pytest.mark.parametrize("F", [8, 3])
def test_sddmm_row_lengths_at_the_default_bounds(ctx, F):
    rng = np.random.default_rng(1)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check_dot(ctx, plan, rowptr, adj, 97, F, rng, "default bounds F=%d" % F)
    plan.close()


@pytest.mark.parametrize("F", [4, 3, 40])
def test_sddmm_row_lengths_under_shrunk_bounds(ctx, monkeypatch, F):
    switches = shrink(monkeypatch)
    rng = np.random.default_rng(2)
    rowptr, adj = csr_of(list(range(131)), 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check_dot(ctx, plan, rowptr, adj, 11, F, rng, "shrunk bounds F=%d" % F, **switches)
    assert plan.info()["hub_rows"] == 131 - 65
    plan.close()


@pytest.fixture(scope="module")
def three_rows():
    rng = np.random.default_rng(3)
    return csr_of([5, 100, 2000], 50, rng)


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 8, 31, 32, 33, 64, 65, 256, 260])
def test_sddmm_widths(ctx, three_rows, F):
    """a short, a wave and a workgroup row; at 260 columns 9 tiles in the short class and 2 in the others"""
    rowptr, adj = three_rows
    plan = plan_of(ctx, rowptr, adj, 50)
    check_dot(ctx, plan, rowptr, adj, 50, F, np.random.default_rng(100 + F), "widths F=%d" % F)
    if F == 260:
        assert plan.last_edge_stats["column_tiles"] == [9, 2, 2]
    plan.close()


def test_sddmm_views_repeats_self_entries(ctx):
    """a view that starts one element off 16 bytes takes the scalar path; column slices go with their leading dimension; a turned view is made
    contiguous; rows that list themselves and one neighbour three times"""
    A = api()
    rng = np.random.default_rng(4)
    rowptr, adj = csr_of(list(range(67)), 67, rng)
    plan = plan_of(ctx, rowptr, adj, 67)
    a, b = ints(rng, 67, 4), ints(rng, 67, 4)
    want = ER.sddmm(rowptr, adj, a, b)[0]
    flat = torch.zeros(67 * 4 + 1, dtype=torch.float32, device=ctx.device)
    view = flat[1:].view(67, 4)
    view.copy_(dev(ctx, a))
    assert view.storage_offset() == 1 and np.array_equal(host(A.sddmm(plan, view, dev(ctx, b))), want) and plan.last_edge_stats["vec"] == 1
    assert np.array_equal(host(A.sddmm(plan, dev(ctx, a), dev(ctx, b))), want) and plan.last_edge_stats["vec"] == 4
    wide = torch.zeros((67, 12), dtype=torch.float32, device=ctx.device)
    for first, vec in ((4, 4), (1, 1)):
        wide.zero_()
        wide[:, first:first + 4] = dev(ctx, b)
        piece = wide[:, first:first + 4]
        assert not piece.is_contiguous() and np.array_equal(host(A.sddmm(plan, dev(ctx, a), piece)), want) and plan.last_edge_stats["vec"] == vec
        assert np.array_equal(host(A.sddmm(plan, piece, dev(ctx, a))), ER.sddmm(rowptr, adj, b, a)[0])
    turned = dev(ctx, np.ascontiguousarray(a.T)).t()
    assert turned.stride(1) != 1 and np.array_equal(host(A.sddmm(plan, turned, dev(ctx, b))), want)
    # the gradients reach the leaves behind slices
    la = torch.zeros((67, 12), dtype=torch.float32, device=ctx.device, requires_grad=True)
    lb = torch.zeros((67, 12), dtype=torch.float32, device=ctx.device, requires_grad=True)
    with torch.no_grad():
        la[:, 4:8] = dev(ctx, a)
        lb[:, 1:5] = dev(ctx, b)
    ge = ints(rng, len(adj))
    A.sddmm(plan, la[:, 4:8], lb[:, 1:5]).backward(dev(ctx, ge))
    ga, gb = ER.sddmm_backward64(rowptr, adj, 67, a, b, ge)
    assert np.array_equal(host(la.grad)[:, 4:8], ga.astype(np.float32)) and not host(la.grad)[:, :4].any() and not host(la.grad)[:, 8:].any()
    assert np.array_equal(host(lb.grad)[:, 1:5], gb.astype(np.float32)) and not host(lb.grad)[:, :1].any() and not host(lb.grad)[:, 5:].any()
    plan.close()
    n = 40
    rows = [[i, i, (i + 1) % n, (i + 1) % n, (i + 1) % n] + [int(v) for v in rng.integers(0, n, i % 7)] for i in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    adj = np.array([v for r in rows for v in r], dtype=np.int32)
    plan = plan_of(ctx, rowptr, adj, n)
    check_dot(ctx, plan, rowptr, adj, n, 5, rng, "repeats and self entries")
    plan.close()


def star(n=40000):
    rowptr = np.zeros(n + 2, dtype=np.int64)
    rowptr[1:] = n
    return rowptr, np.arange(1, n + 1, dtype=np.int32)


def test_in_star_of_40000_entries(ctx):
    """one row of 40 000 entries, three default chunks: the dot products, the softmax through the merge of the chunks, its backward"""
    rng = np.random.default_rng(5)
    rowptr, adj = star()
    plan = plan_of(ctx, rowptr, adj, 40001)
    check_dot(ctx, plan, rowptr, adj, 40001, 4, rng, "in-star")
    info = plan.info()
    assert (info["rows_wg"], info["chunks"], info["hub_rows"]) == (1, 3, 1)
    check_softmax_exact(ctx, plan, rowptr, rng, "in-star")
    check_softmax_backward_exact(ctx, plan, rowptr, rng, "in-star")
    plan.close()


# ---- edge softmax, exact ----
def check_softmax_exact(ctx, plan, rowptr, rng, what):
    A = api()
    row, length = row_index(rowptr), np.diff(rowptr)
    E = int(rowptr[-1])
    e = ((row % 7) - 3).astype(np.float32)                             # constant per row, different between rows
    y = host(A.edge_softmax(plan, dev(ctx, e)))
    assert np.array_equal(y, (np.float32(1) / length[row].astype(np.float32))), what
    # a hashed subset at -inf: 1 / k over the k live entries, 0 at the others; every third row fully masked
    dead = (rng.random(E) < 0.4) | (row % 3 == 1)
    masked = np.where(dead, NEG_INF, e)
    live = np.zeros(len(length), dtype=np.int64)
    np.add.at(live, row, ~dead)
    with np.errstate(divide="ignore"):
        want = np.where(dead, np.float32(0), np.float32(1) / live[row].astype(np.float32)).astype(np.float32)
    y = host(A.edge_softmax(plan, dev(ctx, masked)))
    assert np.array_equal(y, want) and not np.isnan(y).any(), what + " masked"
    assert np.array_equal(y, ER.edge_softmax(rowptr, masked)[0]), what + " restatement"


def test_edge_softmax_exact_at_the_default_bounds(ctx):
    rng = np.random.default_rng(6)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check_softmax_exact(ctx, plan, rowptr, rng, "default bounds")
    check_stats(plan, rowptr, 0, 1)
    plan.close()


def test_edge_softmax_exact_under_shrunk_bounds(ctx, monkeypatch):
    """lengths 0 .. 130 in chunks of 64; a row of 200 whose entries 64 .. 127 are all -inf (a dead chunk in the merge); a row whose only live entry
    sits in its last chunk"""
    A = api()
    switches = shrink(monkeypatch)
    rng = np.random.default_rng(7)
    rowptr, adj = csr_of(list(range(131)) + [200, 200], 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check_softmax_exact(ctx, plan, rowptr, rng, "shrunk bounds")
    check_stats(plan, rowptr, 0, 1, **switches)
    e = np.full(int(rowptr[-1]), 2.5, dtype=np.float32)
    e[rowptr[131] + 64:rowptr[131] + 128] = NEG_INF
    e[rowptr[132]:rowptr[133] - 1] = NEG_INF
    y = host(A.edge_softmax(plan, dev(ctx, e)))
    a, b = y[rowptr[131]:rowptr[132]], y[rowptr[132]:rowptr[133]]
    assert np.array_equal(a[:64], np.full(64, np.float32(1) / np.float32(136))) and not a[64:128].any() and np.array_equal(a[128:], np.full(72, np.float32(1) / np.float32(136)))
    assert not b[:-1].any() and b[-1] == 1.0
    plan.close()


# ---- edge softmax backward, exact ----
def check_softmax_backward_exact(ctx, plan, rowptr, rng, what):
    E = int(rowptr[-1])
    y, gy = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), E), ints(rng, E)
    ge = plan._edge_softmax_backward(dev(ctx, y), dev(ctx, gy))        # the formula on any y: every product and partial sum is exact
    want, exact, _ = ER.edge_softmax_backward(rowptr, y, gy)
    assert np.array_equal(want.astype(np.float64), exact) and np.array_equal(host(ge), want), what


def test_edge_softmax_backward_exact_at_the_default_bounds(ctx):
    rng = np.random.default_rng(8)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check_softmax_backward_exact(ctx, plan, rowptr, rng, "default bounds")
    assert plan.last_edge_stats["algorithmic_bytes"] >= 20 * int(rowptr[-1])
    plan.close()


def test_edge_softmax_backward_exact_under_shrunk_bounds(ctx, monkeypatch):
    shrink(monkeypatch)
    rng = np.random.default_rng(9)
    rowptr, adj = csr_of(list(range(131)), 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check_softmax_backward_exact(ctx, plan, rowptr, rng, "shrunk bounds")
    plan.close()


POWERS = [1, 2, 4, 8, 16, 32, 64, 128, 1024, 2048, 4096, 32768]


def test_edge_softmax_loss_backward_on_rows_of_power_of_two_length(ctx):
    """a constant score per row gives y = 1 / len, a power of two: the gradient through loss.backward() is exact (32768: two default chunks)"""
    A = api()
    rng = np.random.default_rng(10)
    rowptr, adj = csr_of(POWERS, 5, rng)
    plan = plan_of(ctx, rowptr, adj, 5)
    row = row_index(rowptr)
    e = dev(ctx, (row % 5).astype(np.float32)).requires_grad_(True)
    gy = ints(rng, len(adj))
    y = A.edge_softmax(plan, e)
    (y * dev(ctx, gy)).sum().backward()
    want = ER.softmax_backward64(rowptr, 1.0 / np.diff(rowptr)[row], gy)
    assert np.array_equal(host(y).astype(np.float64), 1.0 / np.diff(rowptr)[row]) and np.array_equal(host(e.grad).astype(np.float64), want)
    plan.close()


# ---- real-valued data ----
def test_real_valued_inputs_within_the_bounds_and_the_same_bits_twice(ctx):
    A = api()
    rng = np.random.default_rng(11)
    lengths = LONG + [40000]
    rowptr, adj = csr_of(lengths, 61, rng)
    E, F = len(adj), 8
    a, b = rng.standard_normal((len(lengths), F)).astype(np.float32), rng.standard_normal((61, F)).astype(np.float32)
    e, gy = rng.uniform(-8, 8, E).astype(np.float32), rng.standard_normal(E).astype(np.float32)
    plan = plan_of(ctx, rowptr, adj, 61)

    def within(got, exact, bound, what):
        err = np.abs(got.astype(np.float64) - exact)
        print(what, "largest error", float(err.max(initial=0.0)), "largest bound", float(bound.max(initial=0.0)), "largest error / bound",
              float((err / np.maximum(bound, 1e-300)).max(initial=0.0)))
        assert np.all(err <= bound), what

    runs = []
    for _ in range(2):
        dot = A.sddmm(plan, dev(ctx, a), dev(ctx, b))
        mean = plan._sddmm(dev(ctx, a), dev(ctx, b), 1)
        y = A.edge_softmax(plan, dev(ctx, e))
        ge = plan._edge_softmax_backward(y, dev(ctx, gy))
        runs.append((dot, mean, y, ge))
    assert all(same_bits(p, q) for p, q in zip(*runs))
    dot, mean, y, ge = (host(t) for t in runs[0])
    for got, is_mean in ((dot, False), (mean, True)):
        _, mag, exact = ER.sddmm(rowptr, adj, a, b, mean=is_mean)
        within(got, exact, ER.dot_bound(F) * mag, "dot mean=%d" % is_mean)
    _, exact, R, d = ER.edge_softmax(rowptr, e)
    assert R.max() <= 16
    within(y, exact, ER.softmax_bound(d, R) * exact + ER.TINY, "softmax")
    _, gexact, gmag = ER.edge_softmax_backward(rowptr, y, gy)           # y is data: the device's own
    within(ge, gexact, ER.softmax_backward_bound(d) * gmag, "softmax backward")
    plan.close()


# ---- gradient wiring ----
def test_sddmm_gradients_are_the_two_aggregation_runs(ctx):
    A = api()
    rng = np.random.default_rng(12)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    a, b = rng.standard_normal((len(LONG), 8)).astype(np.float32), rng.standard_normal((97, 8)).astype(np.float32)
    ge = dev(ctx, rng.standard_normal(len(adj)).astype(np.float32))
    at, bt = dev(ctx, a).requires_grad_(True), dev(ctx, b).requires_grad_(True)
    A.sddmm(plan, at, bt).backward(ge)
    assert same_bits(at.grad, A.aggregate(plan, dev(ctx, b), "sum", ge))
    assert same_bits(bt.grad, plan._backward(dev(ctx, a), A.AGG_OPS["sum"], ge, None))
    only = dev(ctx, a).requires_grad_(True)                              # needs_input_grad: b asks for nothing
    A.sddmm(plan, only, dev(ctx, b)).backward(ge)
    assert same_bits(only.grad, at.grad)
    with pytest.raises(lib().VglHipError, match="SDDMM"):
        A.aggregate(plan, dev(ctx, b), "sum", ge.clone().requires_grad_(True))
    plan.close()


@pytest.mark.parametrize("op", ["sum", "mean"])
def test_spmm_gradients_equal_torch_cpu_autograd_on_integer_data(ctx, op):
    A = api()
    rng = np.random.default_rng(13)
    lengths = [0, 1, 2, 5, 9, 33, 40, 70, 0, 3, 1100]
    rowptr, adj = csr_of(lengths, 17, rng)
    w, x, g = rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), len(adj)), ints(rng, 17, 6), ints(rng, len(lengths), 6)
    plan = plan_of(ctx, rowptr, adj, 17)
    wt, xt = dev(ctx, w).requires_grad_(True), dev(ctx, x).requires_grad_(True)
    out = A.spmm(plan, wt, xt, op)
    out.backward(dev(ctx, g))
    wc, xc = torch.tensor(w.astype(np.float64), requires_grad=True), torch.tensor(x.astype(np.float64), requires_grad=True)
    ref = torch.zeros((len(lengths), 6), dtype=torch.float64).index_add_(0, torch.as_tensor(row_index(rowptr)), wc[:, None] * xc[torch.as_tensor(adj.astype(np.int64))])
    if op == "mean":
        ref = ref / torch.as_tensor(np.maximum(lengths, 1)[:, None].astype(np.float64))
    (ref * torch.as_tensor(g.astype(np.float64))).sum().backward()
    assert np.array_equal(host(out), ref.detach().numpy().astype(np.float32))
    assert np.array_equal(host(wt.grad), wc.grad.numpy().astype(np.float32)), "grad weight"       # an integer dot product, one division
    if op == "sum":
        assert np.array_equal(host(xt.grad), xc.grad.numpy().astype(np.float32)), "grad x"
    else:
        _, gmag, gexact = AR.backward(rowptr, adj, 17, g, "mean", w, with_abs=True)
        assert np.all(np.abs(host(xt.grad) - gexact) <= AR.tolerance(int(np.bincount(adj, minlength=17).max())) * gmag), "grad x"
    plan.close()


# ---- attention, end to end ----
def test_graph_attention_is_its_three_parts(ctx):
    A = api()
    rng = np.random.default_rng(14)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    q, k, v = (rng.standard_normal(s).astype(np.float32) * 0.5 for s in ((len(LONG), 8), (97, 8), (97, 5)))
    g = dev(ctx, rng.standard_normal((len(LONG), 5)).astype(np.float32))
    grads = []
    for whole in (True, False):
        qt, kt, vt = (dev(ctx, t).requires_grad_(True) for t in (q, k, v))
        if whole:
            out, w = A.graph_attention(plan, qt, kt, vt, return_weights=True)
        else:
            w = A.edge_softmax(plan, A.sddmm(plan, qt, kt) * (8 ** -0.5))
            out = A.spmm(plan, w, vt)
        out.backward(g)
        grads.append((out.detach(), w.detach(), qt.grad, kt.grad, vt.grad))
    assert all(same_bits(p, r) for p, r in zip(*grads))
    half = A.graph_attention(plan, dev(ctx, q), dev(ctx, k), dev(ctx, v), scale=0.5)
    assert same_bits(half, A.spmm(plan, A.edge_softmax(plan, A.sddmm(plan, dev(ctx, q), dev(ctx, k)) * 0.5), dev(ctx, v)))
    plan.close()


def test_graph_attention_exact_with_q_zero_on_rows_of_power_of_two_length(ctx, monkeypatch):
    """q = 0: every weight is 1 / len, a power of two, and with integer k, v, g every gradient is a sum of dyadic numbers: out, grad q, grad k and
    grad v equal torch CPU float64 autograd exactly.  Lengths 1 .. 128 = 2^l under the shrunk bounds (every class, 128: two chunks) and integers in
    [-4, 4] keep every partial sum exact in float32: the widest, grad q, has terms that are multiples of 2^-(2 l + 1) and partial sums below 2^8,
    9 + 2 l <= 23 bits."""
    A = api()
    shrink(monkeypatch)
    rng = np.random.default_rng(15)
    lengths = [1, 2, 4, 8, 16, 32, 64, 128, 0, 128]
    rowptr, adj = csr_of(lengths, 23, rng)
    n, F = len(lengths), 4
    k, v, g = (rng.integers(-4, 5, s).astype(np.float32) for s in ((23, F), (23, 3), (n, 3)))
    plan = plan_of(ctx, rowptr, adj, 23)
    qt, kt, vt = torch.zeros((n, F), device=ctx.device, requires_grad=True), dev(ctx, k).requires_grad_(True), dev(ctx, v).requires_grad_(True)
    out = A.graph_attention(plan, qt, kt, vt)
    out.backward(dev(ctx, g))
    qc, kc, vc = torch.zeros((n, F), dtype=torch.float64, requires_grad=True), torch.tensor(k.astype(np.float64), requires_grad=True), torch.tensor(v.astype(np.float64), requires_grad=True)
    row, a = torch.as_tensor(row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    e = (qc[row] * kc[a]).sum(-1) * 0.5
    w = torch.cat([torch.softmax(e[rowptr[i]:rowptr[i + 1]], 0) for i in range(n)])
    ref = torch.zeros((n, 3), dtype=torch.float64).index_add_(0, row, w[:, None] * vc[a])
    (ref * torch.as_tensor(g.astype(np.float64))).sum().backward()
    for got, want, what in ((out, ref.detach(), "out"), (qt.grad, qc.grad, "grad q"), (kt.grad, kc.grad, "grad k"), (vt.grad, vc.grad, "grad v")):
        assert np.array_equal(host(got).astype(np.float64), want.numpy()), what
    assert qc.grad.abs().sum() > 0 and vc.grad.abs().sum() > 0
    plan.close()


def test_sampled_blocks_two_layer_attention_chain(ctx):
    """sample_blocks on RMAT-10 x 8, two hops, from_block; each layer attends from a block's seeds over its sampled entries; forward, layer by layer,
    within the bound composed in edge_reference.attention (the input of a layer is data: the device's own)"""
    A = api()
    rng = np.random.default_rng(16)
    src, dst = ctx.gen_rmat(10, 8, 5)
    g = A.Graph.from_coo(ctx, 1 << 10, src, dst)
    seeds = torch.tensor(rng.choice(1 << 10, 64, replace=False).astype(np.int32), device=ctx.device)
    blocks = A.sample_blocks(g, seeds, [6, 4], seed=11, direction="in")
    (p0, cols0), (p1, cols1) = A.AggregationPlan.from_block(ctx, blocks[0]), A.AggregationPlan.from_block(ctx, blocks[1])
    assert torch.equal(cols0, blocks[1]["seeds"])
    F = 8
    x = dev(ctx, (rng.standard_normal((p1.n_cols, F)) * 0.5).astype(np.float32))
    at1, at0 = torch.searchsorted(cols1, blocks[1]["seeds"]).long(), torch.searchsorted(cols0, blocks[0]["seeds"]).long()
    h1 = A.graph_attention(p1, x[at1], x, x)
    h0 = A.graph_attention(p0, h1[at0], h1, h1)
    assert tuple(h1.shape) == (cols0.numel(), F) and tuple(h0.shape) == (64, F)
    for p, q, kv, got, what in ((p1, x[at1], x, h1, "layer 1"), (p0, h1[at0], h1, h0, "layer 0")):
        r = ER.attention(host(p.rowptr), host(p.adj), host(q), host(kv), host(kv))
        err = np.abs(host(got).astype(np.float64) - r["out"])
        print(what, "largest error", float(err.max()), "largest bound", float(r["bound"].max()))
        assert np.all(err <= r["bound"]), what
    p0.close(); p1.close(); g.close()


# ---- housekeeping ----
def test_plan_run_destroy_three_times(ctx):
    A = api()
    rng = np.random.default_rng(17)
    rowptr, adj = csr_of(LONG, 97, rng)
    q, k, v = (rng.standard_normal(s).astype(np.float32) * 0.5 for s in ((len(LONG), 4), (97, 4), (97, 4)))
    seen = []
    for _ in range(3):
        plan = plan_of(ctx, rowptr, adj, 97)
        qt = dev(ctx, q).requires_grad_(True)
        out, w = A.graph_attention(plan, qt, dev(ctx, k), dev(ctx, v), return_weights=True)
        out.sum().backward()
        seen.append((out.detach().clone(), w.detach().clone(), qt.grad.clone()))
        plan.close()
        assert plan.h is None
    for other in seen[1:]:
        assert all(same_bits(a, b) for a, b in zip(seen[0], other))


def test_python_refusals(ctx):
    A, L = api(), lib()
    rng = np.random.default_rng(18)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    a, b, e = dev(ctx, ints(rng, 3, 3)), dev(ctx, ints(rng, 4, 3)), dev(ctx, ints(rng, 5))
    for bad, match in ((lambda: A.sddmm(plan, a.double(), b), "float64"), (lambda: A.sddmm(plan, a, b.half()), "float16"),
                       (lambda: A.sddmm(plan, a[:2], b), "n_rows x F"), (lambda: A.sddmm(plan, a, b[:3]), "n_cols x F"),
                       (lambda: A.sddmm(plan, a[:, 0], b), "n_rows x F"), (lambda: A.sddmm(plan, a, b[:, :2]), "same width"),
                       (lambda: A.sddmm(plan, a.cpu(), b), "device"), (lambda: A.edge_softmax(plan, e.double()), "float64"),
                       (lambda: A.edge_softmax(plan, e[:4]), "one value per entry"), (lambda: A.edge_softmax(plan, e.cpu()), "one value per entry"),
                       (lambda: A.edge_softmax(plan, e.view(5, 1)), "one value per entry"), (lambda: A.spmm(plan, e, b, "max"), "'sum' or 'mean'"),
                       (lambda: A.spmm(plan, e.int(), b), "int32"), (lambda: A.spmm(plan, e[:4], b), "one value per entry"),
                       (lambda: A.spmm(plan, e, b[:3]), "n_cols x F"), (lambda: A.graph_attention(plan, a, b, b[:3]), "n_cols x F"),
                       (lambda: A.graph_attention(plan, a.double(), b, b), "float64")):
        with pytest.raises(L.VglHipError, match=match):
            bad()
    plan.close()
    for bad in (lambda: A.sddmm(plan, a, b), lambda: A.edge_softmax(plan, e), lambda: A.spmm(plan, e, b), lambda: A.graph_attention(plan, a, b, b)):
        with pytest.raises(L.VglHipError, match="open AggregationPlan"):
            bad()


def test_c_refusals_come_before_any_write(ctx):
    A, L = api(), lib()
    lb = ctx.L
    rng = np.random.default_rng(19)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    h = plan.h
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    a, b = dev(ctx, ints(rng, 3, 4)), dev(ctx, ints(rng, 4, 4))
    e, y, ge = (torch.full((5,), 77.0, device=ctx.device) for _ in range(3))
    other = A.Context(0)
    dot, sm, back = lb.vgl_hip_agg_sddmm, lb.vgl_hip_agg_edge_softmax, lb.vgl_hip_agg_edge_softmax_backward
    refused = [
        dot(None, h, ptr(a), 4, ptr(b), 4, 4, 0, ptr(e), None), dot(ctx.h, None, ptr(a), 4, ptr(b), 4, 4, 0, ptr(e), None),
        dot(ctx.h, h, None, 4, ptr(b), 4, 4, 0, ptr(e), None), dot(ctx.h, h, ptr(a), 4, None, 4, 4, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 0, None, None), dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 0, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 3, ptr(b), 4, 4, 0, ptr(e), None), dot(ctx.h, h, ptr(a), 4, ptr(b), 3, 4, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 2, ptr(e), None), dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, -1, ptr(e), None),
        dot(other.h, h, ptr(a), 4, ptr(b), 4, 4, 0, ptr(e), None),
        sm(None, h, ptr(ge), ptr(y), None), sm(ctx.h, None, ptr(ge), ptr(y), None), sm(ctx.h, h, None, ptr(y), None), sm(ctx.h, h, ptr(ge), None, None),
        sm(other.h, h, ptr(ge), ptr(y), None),
        back(None, h, ptr(y), ptr(e), ptr(ge), None), back(ctx.h, None, ptr(y), ptr(e), ptr(ge), None), back(ctx.h, h, None, ptr(e), ptr(ge), None),
        back(ctx.h, h, ptr(y), None, ptr(ge), None), back(ctx.h, h, ptr(y), ptr(e), None, None), back(other.h, h, ptr(y), ptr(e), ptr(ge), None),
    ]
    assert all(rc != 0 for rc in refused), refused
    assert b"another context" in lb.vgl_hip_last_error()
    ctx.sync()
    assert (e == 77.0).all() and (y == 77.0).all() and (ge == 77.0).all()
    st = L.AggStats()
    assert dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 0, ptr(e), C.byref(st)) == 0 and st.rows == 3 and st.entries == 5 and st.vec == 4 and st.transposed == 0
    assert np.array_equal(host(e), ER.sddmm(rowptr, adj, host(a), host(b))[0])
    # the model, term by term: the adjacency per tile, b gathered and e written per entry, the bounds and a per row, the list entries
    assert st.algorithmic_bytes == 5 * 4 + 5 * (4 * 4 + 4) + 3 * (8 + 4 * 4) + 3 * 4
    assert sm(ctx.h, h, ptr(e), ptr(y), C.byref(st)) == 0 and st.algorithmic_bytes == 5 * (4 * 3 + 4) + 3 * 8 + 3 * 4 and list(st.column_tiles) == [1, 1, 1]
    assert back(ctx.h, h, ptr(y), ptr(e), ptr(ge), C.byref(st)) == 0 and st.algorithmic_bytes == 5 * (8 * 2 + 4) + 3 * 8 + 3 * 4 and st.vec == 1
    other.close()
    plan.close()


def test_empty_shapes(ctx):
    """no entries, no rows, no columns of features: empty or zero tensors of the right shape, and gradients of the right shape"""
    A = api()
    plan = plan_of(ctx, np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), 2)
    q, k = torch.ones((3, 3), device=ctx.device, requires_grad=True), torch.ones((2, 3), device=ctx.device, requires_grad=True)
    e = A.sddmm(plan, q, k)
    assert tuple(e.shape) == (0,) and tuple(A.edge_softmax(plan, e).shape) == (0,)
    out = A.graph_attention(plan, q, k, k)
    assert out.tolist() == [[0.0] * 3] * 3
    out.sum().backward()
    assert q.grad.tolist() == [[0.0] * 3] * 3 and k.grad.tolist() == [[0.0] * 3] * 2
    plan.close()
    plan = plan_of(ctx, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 2)
    assert tuple(A.graph_attention(plan, torch.ones((0, 3), device=ctx.device), torch.ones((2, 3), device=ctx.device), torch.ones((2, 3), device=ctx.device)).shape) == (0, 3)
    plan.close()
    rng = np.random.default_rng(20)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    e = A.sddmm(plan, torch.ones((3, 0), device=ctx.device), torch.ones((4, 0), device=ctx.device))
    assert e.tolist() == [0.0] * 5
    assert tuple(A.spmm(plan, torch.ones(5, device=ctx.device), torch.ones((4, 0), device=ctx.device)).shape) == (3, 0)
    plan.close()


@pytest.mark.parametrize("extra", [[], ["-backward", "-features", "12"], ["-stage", "softmax", "-backward", "-out"]])
def test_app_check(extra):
    cmd = [os.path.join(ROOT, "apps", "bin", "attn_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "ATTN launches:" in out.stdout, out.stdout
