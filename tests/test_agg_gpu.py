"""Neighbour aggregation on the GPU (vgl_hip_agg_*, api.AggregationPlan / aggregate / aggregate_neighbors, apps/bin/agg_hip) against the numpy
restatement of the contract (tests/agg_reference.py).  Almost every comparison is on integer-valued data (x in [-8, 8], weights in {0.5, 1, 2}, every
partial sum far below 2^24), where every shape of a float32 sum gives the same bits, so results are compared for EQUALITY: a lost entry, a leaking
column or a wrong chunk cannot hide in a tolerance.  MEAN forward is equal too (one correctly rounded division of an exact sum); MEAN backward has
the inexact coefficient w / len and is compared within agg_reference.tolerance(d) like the real-valued inputs.  The arg is always compared for
equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import agg_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHRUNK = {"VGL_AGG_SHORT": "4", "VGL_AGG_WAVE": "16", "VGL_AGG_CHUNK": "64"}
CASES = [("sum", False), ("sum", True), ("mean", False), ("mean", True), ("max", False), ("min", False)]


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


def ints(rng, n, F):
    return rng.integers(-8, 9, (n, F)).astype(np.float32)


def weights(rng, E):
    return rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), E)


def dev(ctx, a):
    return torch.tensor(a, device=ctx.device)


def plan_of(ctx, rowptr, adj, n_cols):
    return api().AggregationPlan(ctx, dev(ctx, rowptr), dev(ctx, adj), n_cols)


def within(got, exact, mag, d, what):
    err, bound = np.abs(got.astype(np.float64) - exact), R.tolerance(d) * mag
    print(what, "largest error", float(err.max(initial=0.0)), "largest bound", float(bound.max(initial=0.0)), "d", d)
    assert np.all(err <= bound), what


def check(ctx, plan, rowptr, adj, n_cols, x, g, w, cases=CASES, exact=True, what=""):
    """forward and backward of every case through the API against the restatement: equality on integer-valued data (exact), else the tolerance"""
    A = api()
    length = np.diff(rowptr)
    d_fwd = int(length.max(initial=0))
    d_bwd = int(np.bincount(adj, minlength=n_cols).max(initial=0))
    for op, weighted in cases:
        wt = dev(ctx, w) if weighted else None
        xt = dev(ctx, x).requires_grad_(True)
        out, arg = A.aggregate(plan, xt, op, wt, return_arg=True)
        want, want_arg, mag, exact64 = R.forward(rowptr, adj, x, op, w if weighted else None, with_abs=True)
        tag = "%s %s%s F=%d" % (what, op, " weighted" if weighted else "", x.shape[1])
        assert out.dtype == torch.float32 and tuple(out.shape) == want.shape, tag
        if exact:
            assert np.array_equal(out.detach().cpu().numpy(), want), tag
        else:
            within(out.detach().cpu().numpy(), exact64, mag, d_fwd, tag)
        if want_arg is None:
            assert arg is None, tag
        else:
            assert arg.dtype == torch.int32 and np.array_equal(arg.cpu().numpy(), want_arg), tag
        out.backward(dev(ctx, g))
        gx, gmag, gexact = R.backward(rowptr, adj, n_cols, g, op, w if weighted else None, want_arg, with_abs=True)
        got = xt.grad.cpu().numpy()
        if exact and op != "mean":
            assert np.array_equal(got, gx), tag + " backward"
        else:
            within(got, gexact, gmag, d_bwd, tag + " backward")


def check_stats(plan, rowptr, adj, n_cols, F, vec, **switches):
    want = R.classify(rowptr, **switches)
    info = plan.info()
    for k, v in want.items():
        assert info[k] == v and plan.last_stats[k] == v, (k, info[k], plan.last_stats[k], v)
    assert plan.last_stats["column_tiles"] == R.column_tiles(F, vec) and plan.last_stats["vec"] == vec and plan.last_stats["transposed"] == 0
    t_rowptr, _, _ = R.transpose(rowptr, adj, n_cols)
    back = plan.last_backward_stats
    for k, v in R.classify(t_rowptr, **switches).items():
        assert back[k] == v, ("transposed", k, back[k], v)
    assert back["transposed"] == 1 and plan.info()["transposed"] == 1 and back["column_tiles"] == R.column_tiles(F, vec)
    assert plan.last_stats["algorithmic_bytes"] > 4 * want["entries"] * F and back["algorithmic_bytes"] > 4 * want["entries"] * F


LONG = list(range(67)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


@pytest.mark.parametrize("F", [8, 3])
def test_row_lengths_at_the_default_bounds(ctx, F):
    """every length 0 .. 66, 255 - 257, 1023 - 1025 and 4095 - 4097: all three classes; 97 columns, so the transposed rows are of the wave class"""
    rng = np.random.default_rng(1)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check(ctx, plan, rowptr, adj, 97, ints(rng, 97, F), ints(rng, len(LONG), F), weights(rng, len(adj)), what="default bounds")
    check_stats(plan, rowptr, adj, 97, F, 4 if F % 4 == 0 else 1)
    plan.close()


@pytest.mark.parametrize("F", [4, 3, 40])
def test_row_lengths_under_shrunk_bounds(ctx, monkeypatch, F):
    """lengths 0 .. 130 with short <= 4, wave <= 16 and chunks of 64: every class edge and several chunk edges are crossed by tiny rows, and with 11
    columns the transposed rows have a dozen chunks each"""
    for k, v in SHRUNK.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(2)
    lengths = list(range(131))
    rowptr, adj = csr_of(lengths, 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check(ctx, plan, rowptr, adj, 11, ints(rng, 11, F), ints(rng, 131, F), weights(rng, len(adj)), what="shrunk bounds")
    check_stats(plan, rowptr, adj, 11, F, 4 if F % 4 == 0 else 1, short=4, wave=16, chunk=64)
    assert plan.info()["hub_rows"] == 131 - 65 and plan.last_backward_stats["hub_rows"] == 11
    plan.close()


def test_in_star_of_40000_leaves(ctx):
    """one row of 40 000 entries: three default chunks and the hub kernel in the forward pass; the leaves' gradients are single terms"""
    rng = np.random.default_rng(3)
    n = 40001
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = n - 1
    adj = np.arange(1, n, dtype=np.int32)
    plan = plan_of(ctx, rowptr, adj, n)
    check(ctx, plan, rowptr, adj, n, ints(rng, n, 4), ints(rng, n, 4), weights(rng, n - 1), what="in-star")
    info = plan.info()
    assert (info["rows_wg"], info["chunks"], info["hub_rows"]) == (1, 3, 1)
    plan.close()


def test_one_column_that_40000_rows_read(ctx):
    """the star transposed in role: the backward pass has one transposed row of 40 000 entries (three chunks, the hub kernel)"""
    rng = np.random.default_rng(4)
    n = 40000
    rowptr = np.arange(n + 1, dtype=np.int64)
    adj = np.zeros(n, dtype=np.int32)
    plan = plan_of(ctx, rowptr, adj, 3)
    check(ctx, plan, rowptr, adj, 3, ints(rng, 3, 4), ints(rng, n, 4), weights(rng, n), what="hub column")
    back = plan.last_backward_stats
    assert (back["rows"], back["rows_wg"], back["chunks"], back["hub_rows"]) == (3, 1, 3, 1)
    plan.close()


@pytest.fixture(scope="module")
def short_csr():
    rng = np.random.default_rng(5)
    rowptr, adj = csr_of(list(range(67)), 50, rng)
    return rowptr, adj, rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), len(adj))


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 8, 31, 32, 33, 64, 65, 256, 260])
def test_widths(ctx, short_csr, F):
    """one column, fewer columns than a lane group, one more than a tile of the short class (32 / 8), of the wave class (256 / 64), scalar and vector"""
    rowptr, adj, w = short_csr
    rng = np.random.default_rng(100 + F)
    plan = plan_of(ctx, rowptr, adj, 50)
    check(ctx, plan, rowptr, adj, 50, ints(rng, 50, F), ints(rng, 67, F), w, cases=[("sum", True), ("mean", False), ("max", False)], what="widths")
    assert plan.last_stats["vec"] == (4 if F % 4 == 0 else 1) and plan.last_stats["column_tiles"] == R.column_tiles(F, plan.last_stats["vec"])
    plan.close()


def test_views_offset_by_one_element_and_column_slices(ctx, short_csr):
    """a view whose storage starts one element off 16 bytes takes the scalar path at F = 4; a column slice goes with its leading dimension, unaligned
    slices scalar; a transposed view is made contiguous: all equal to the plain call"""
    A = api()
    rowptr, adj, w = short_csr
    rng = np.random.default_rng(6)
    x = ints(rng, 50, 4)
    plan = plan_of(ctx, rowptr, adj, 50)
    want = R.forward(rowptr, adj, x, "sum", w)[0]
    wt = dev(ctx, w)
    flat = torch.zeros(50 * 4 + 1, dtype=torch.float32, device=ctx.device)
    view = flat[1:].view(50, 4)
    view.copy_(dev(ctx, x))
    assert view.storage_offset() == 1 and np.array_equal(A.aggregate(plan, view, "sum", wt).cpu().numpy(), want)
    assert plan.last_stats["vec"] == 1
    wide = torch.zeros((50, 12), dtype=torch.float32, device=ctx.device)
    for first, vec in ((4, 4), (1, 1)):
        wide.zero_()
        wide[:, first:first + 4] = dev(ctx, x)
        piece = wide[:, first:first + 4]
        assert not piece.is_contiguous() and np.array_equal(A.aggregate(plan, piece, "sum", wt).cpu().numpy(), want)
        assert plan.last_stats["vec"] == vec
        arg = A.aggregate(plan, piece, "max", return_arg=True)[1]
        assert np.array_equal(arg.cpu().numpy(), R.forward(rowptr, adj, x, "max")[1])
    turned = dev(ctx, np.ascontiguousarray(x.T)).t()
    assert turned.stride(1) != 1 and np.array_equal(A.aggregate(plan, turned, "sum", wt).cpu().numpy(), want)
    # the gradient reaches the leaf behind a slice
    leaf = torch.zeros((50, 12), dtype=torch.float32, device=ctx.device, requires_grad=True)
    g = ints(rng, 67, 4)
    A.aggregate(plan, leaf[:, 4:8], "sum", wt).backward(dev(ctx, g))
    grad = leaf.grad.cpu().numpy()
    assert np.array_equal(grad[:, 4:8], R.backward(rowptr, adj, 50, g, "sum", w)) and not grad[:, :4].any() and not grad[:, 8:].any()
    plan.close()


def test_ties_repeated_entries_and_self_entries(ctx):
    """constant columns: the arg is the row's first position whatever the class; rows that list themselves and one neighbour three times"""
    A = api()
    rng = np.random.default_rng(7)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    x = np.full((97, 8), 3.0, dtype=np.float32)
    first = np.where(np.diff(rowptr) > 0, rowptr[:-1], -1).astype(np.int32)
    for op in ("max", "min"):
        out, arg = A.aggregate(plan, dev(ctx, x), op, return_arg=True)
        assert np.array_equal(arg.cpu().numpy(), np.repeat(first[:, None], 8, axis=1))
        assert np.array_equal(out.cpu().numpy(), np.where(first[:, None] >= 0, 3.0, 0.0).astype(np.float32).repeat(8, axis=1))
    plan.close()
    n = 40
    rows = [[i, i, (i + 1) % n, (i + 1) % n, (i + 1) % n] + [int(v) for v in rng.integers(0, n, i % 7)] for i in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    adj = np.array([v for r in rows for v in r], dtype=np.int32)
    plan = plan_of(ctx, rowptr, adj, n)
    check(ctx, plan, rowptr, adj, n, ints(rng, n, 5), ints(rng, n, 5), weights(rng, len(adj)), what="repeats and self entries")
    plan.close()


@pytest.mark.parametrize("op,weighted", CASES)
def test_loss_backward_matches_torch_cpu_autograd(ctx, op, weighted):
    """the same data through loss.backward() here and through torch CPU autograd on index_add_ / per-row max in float64; real-valued, so no ties"""
    A = api()
    rng = np.random.default_rng(8)
    rowptr, adj = csr_of([0, 1, 2, 5, 9, 33, 40, 70, 0, 3], 17, rng)
    x, c = rng.standard_normal((17, 6)).astype(np.float32), rng.standard_normal((10, 6)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, len(adj)).astype(np.float32) if weighted else None
    plan = plan_of(ctx, rowptr, adj, 17)
    xt = dev(ctx, x).requires_grad_(True)
    loss = (A.aggregate(plan, xt, op, dev(ctx, w) if weighted else None) * dev(ctx, c)).sum()
    loss.backward()
    xc = torch.tensor(x.astype(np.float64), requires_grad=True)
    row = torch.repeat_interleave(torch.arange(10), torch.as_tensor(np.diff(rowptr)))
    a = torch.as_tensor(adj.astype(np.int64))
    if op in ("sum", "mean"):
        terms = xc[a] * (torch.as_tensor(w.astype(np.float64))[:, None] if weighted else 1.0)
        ref = torch.zeros((10, 6), dtype=torch.float64).index_add_(0, row, terms)
        if op == "mean":
            ref = ref / torch.as_tensor(np.maximum(np.diff(rowptr), 1)[:, None].astype(np.float64))
    else:
        ref = torch.stack([(xc[a[rowptr[i]:rowptr[i + 1]]].max(0).values if op == "max" else xc[a[rowptr[i]:rowptr[i + 1]]].min(0).values)
                           if rowptr[i + 1] > rowptr[i] else torch.zeros(6, dtype=torch.float64) for i in range(10)])
    (ref * torch.as_tensor(c.astype(np.float64))).sum().backward()
    _, gmag, _ = R.backward(rowptr, adj, 17, c, op, w, R.forward(rowptr, adj, x, op, w)[1], with_abs=True)
    within(xt.grad.cpu().numpy(), xc.grad.numpy(), gmag, int(np.bincount(adj, minlength=17).max()), "loss.backward %s" % op)
    plan.close()


def test_sampled_blocks_two_layer_mean_chain(ctx):
    """sample_blocks on RMAT-10 x 8, two hops; from_block; a two-layer chain of mean aggregations, forward and backward, layer by layer against the
    restatement; cols of hop h are the seeds of hop h + 1"""
    A = api()
    rng = np.random.default_rng(9)
    src, dst = ctx.gen_rmat(10, 8, 5)
    g = A.Graph.from_coo(ctx, 1 << 10, src, dst)
    seeds = torch.tensor(rng.choice(1 << 10, 64, replace=False).astype(np.int32), device=ctx.device)
    blocks = A.sample_blocks(g, seeds, [6, 4], seed=11, direction="in")
    (p0, cols0), (p1, cols1) = A.AggregationPlan.from_block(ctx, blocks[0]), A.AggregationPlan.from_block(ctx, blocks[1])
    assert torch.equal(cols0, blocks[1]["seeds"])
    assert p1.n_rows == cols0.numel() and p0.n_rows == 64 and p1.n_cols == cols1.numel()
    assert torch.equal(cols1[p1.adj.long()], blocks[1]["adj"]) and torch.equal(cols0[p0.adj.long()], blocks[0]["adj"])
    F = 8
    x = ints(rng, p1.n_cols, F)
    xt = dev(ctx, x).requires_grad_(True)
    h1 = A.aggregate(p1, xt, "mean")
    h1.retain_grad()
    h0 = A.aggregate(p0, h1, "mean")
    g0 = ints(rng, 64, F)
    h0.backward(dev(ctx, g0))
    rp1, a1, rp0, a0 = (t.cpu().numpy() for t in (p1.rowptr, p1.adj, p0.rowptr, p0.adj))
    assert np.array_equal(h1.detach().cpu().numpy(), R.forward(rp1, a1, x, "mean")[0])          # integer sums, one division
    h1n = h1.detach().cpu().numpy()
    _, _, mag, exact = R.forward(rp0, a0, h1n, "mean", with_abs=True)
    within(h0.detach().cpu().numpy(), exact, mag, int(np.diff(rp0).max()), "layer 0 forward")
    _, gmag, gexact = R.backward(rp0, a0, p0.n_cols, g0, "mean", with_abs=True)
    within(h1.grad.cpu().numpy(), gexact, gmag, int(np.bincount(a0, minlength=p0.n_cols).max()), "layer 0 backward")
    _, gmag, gexact = R.backward(rp1, a1, p1.n_cols, h1.grad.cpu().numpy(), "mean", with_abs=True)
    within(xt.grad.cpu().numpy(), gexact, gmag, int(np.bincount(a1, minlength=p1.n_cols).max()), "layer 1 backward")
    p0.close(); p1.close(); g.close()


def test_aggregate_neighbors_on_a_renumbered_graph_in_original_order(ctx):
    A = api()
    rng = np.random.default_rng(10)
    V = 1 << 9
    src, dst = ctx.gen_rmat(9, 8, 2)
    plain, sorted_ = A.Graph.from_coo(ctx, V, src, dst), A.Graph.from_coo(ctx, V, src, dst, renumber="out")
    x = ints(rng, V, 8)
    s, d = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64)
    for direction, (row, col) in (("in", (d, s)), ("out", (s, d))):
        want = np.zeros((V, 8))
        np.add.at(want, row, x[col].astype(np.float64))
        for op in ("sum", "mean", "max"):
            a, b = A.aggregate_neighbors(plain, dev(ctx, x), op, direction=direction), A.aggregate_neighbors(sorted_, dev(ctx, x), op, direction=direction)
            assert torch.equal(a, b), (direction, op)
        assert np.array_equal(A.aggregate_neighbors(sorted_, dev(ctx, x), "sum", direction=direction).cpu().numpy(), want.astype(np.float32))
    own = A.aggregate_neighbors(sorted_, dev(ctx, x)[sorted_.bwd.long()], "sum", raw=True)
    assert torch.equal(own[sorted_.fwd.long()], A.aggregate_neighbors(plain, dev(ctx, x), "sum"))
    assert set(sorted_._agg_plans) == {"in", "out"}
    kept = list(sorted_._agg_plans.values())
    plain.close(); sorted_.close()
    assert all(p.h is None for p in kept)


def test_real_valued_inputs_within_the_tolerance_and_the_same_bits_twice(ctx):
    """standard normal features and uniform weights on rows of every class (a row of 40 000 among them): within tolerance(d) of the float64 result per
    value, d the longest row; the same call again returns the same bits, forward and backward"""
    A = api()
    rng = np.random.default_rng(11)
    lengths = LONG + [40000]
    rowptr, adj = csr_of(lengths, 61, rng)
    x, g = rng.standard_normal((61, 8)).astype(np.float32), rng.standard_normal((len(lengths), 8)).astype(np.float32)
    w = rng.uniform(0.5, 2.0, len(adj)).astype(np.float32)
    plan = plan_of(ctx, rowptr, adj, 61)
    check(ctx, plan, rowptr, adj, 61, x, g, w, exact=False, what="real-valued")
    for op, weighted in CASES:
        runs = []
        for _ in range(2):
            xt = dev(ctx, x).requires_grad_(True)
            out = A.aggregate(plan, xt, op, dev(ctx, w) if weighted else None)
            out.backward(dev(ctx, g))
            runs.append((out.detach().clone(), xt.grad.clone()))
        assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), op
    plan.close()


def test_plan_run_destroy_three_times(ctx):
    A = api()
    rng = np.random.default_rng(12)
    rowptr, adj = csr_of(LONG, 97, rng)
    x, g = rng.standard_normal((97, 4)).astype(np.float32), rng.standard_normal((len(LONG), 4)).astype(np.float32)
    seen = []
    for _ in range(3):
        plan = plan_of(ctx, rowptr, adj, 97)
        xt = dev(ctx, x).requires_grad_(True)
        out, arg = A.aggregate(plan, xt, "max", return_arg=True)
        out.backward(dev(ctx, g))
        s = A.aggregate(plan, dev(ctx, x), "sum")
        seen.append((out.detach().clone(), arg.clone(), xt.grad.clone(), s.clone()))
        plan.close()
        assert plan.h is None
    for other in seen[1:]:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(seen[0], other))


def test_python_refusals(ctx):
    A, L = api(), lib()
    rng = np.random.default_rng(13)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    x = dev(ctx, ints(rng, 4, 3))
    with pytest.raises(L.VglHipError, match="float64"):
        A.aggregate(plan, x.double())
    with pytest.raises(L.VglHipError, match="float16"):
        A.aggregate(plan, x.half())
    with pytest.raises(L.VglHipError, match="int32"):
        A.aggregate(plan, x.int())
    with pytest.raises(L.VglHipError, match="float64"):
        A.aggregate(plan, x, weight=torch.ones(5, dtype=torch.float64, device=ctx.device))
    with pytest.raises(L.VglHipError, match="SDDMM"):
        A.aggregate(plan, x, weight=torch.ones(5, device=ctx.device, requires_grad=True))
    with pytest.raises(L.VglHipError, match="no entry weights"):
        A.aggregate(plan, x, "max", weight=torch.ones(5, device=ctx.device))
    with pytest.raises(L.VglHipError, match="op must be"):
        A.aggregate(plan, x, "median")
    with pytest.raises(L.VglHipError, match="n_cols x F"):
        A.aggregate(plan, x[:3])
    with pytest.raises(L.VglHipError, match="one value per entry"):
        A.aggregate(plan, x, weight=torch.ones(4, device=ctx.device))
    with pytest.raises(L.VglHipError, match="rowptr ends at"):
        A.AggregationPlan(ctx, dev(ctx, rowptr), dev(ctx, adj[:-1]), 4)
    with pytest.raises(L.VglHipError, match="int64"):
        A.AggregationPlan(ctx, dev(ctx, rowptr.astype(np.int32)), dev(ctx, adj), 4)
    plan.close()
    with pytest.raises(L.VglHipError, match="open AggregationPlan"):
        A.aggregate(plan, x)


def test_c_refusals_come_before_any_write(ctx):
    """every refusal of the C entry points; the outputs keep the pattern they were given"""
    A, L = api(), lib()
    lb = ctx.L
    rng = np.random.default_rng(14)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def create(rp, ad, n_rows, n_cols, out=True):
        h = C.c_void_p()
        rc = lb.vgl_hip_agg_plan_create(ctx.h, ptr(rp) if rp is not None else None, ptr(ad) if ad is not None else None, n_rows, n_cols, C.byref(h) if out else None)
        return rc, h

    rp, ad = dev(ctx, rowptr), dev(ctx, adj)
    for bad in (create(None, ad, 3, 4), create(rp, None, 3, 4), create(rp, ad, 3, 4, out=False), create(rp, ad, -1, 4), create(rp, ad, 3, -1),
                create(dev(ctx, np.array([0, 2, 1, 5], dtype=np.int64)), ad, 3, 4), create(dev(ctx, np.array([1, 2, 2, 5], dtype=np.int64)), ad, 3, 4),
                create(rp, ad, 3, int(adj.max())), create(rp, dev(ctx, np.array([0, 1, -1, 2, 3], dtype=np.int32)), 3, 4)):
        assert bad[0] != 0 and not bad[1].value
    assert b"rowptr" in lb.vgl_hip_last_error() or b"adj" in lb.vgl_hip_last_error()
    rc, h = create(rp, ad, 3, 4)
    assert rc == 0 and h.value
    x, w = dev(ctx, ints(rng, 4, 4)), torch.ones(5, device=ctx.device)
    out = torch.full((3, 4), 77.0, device=ctx.device)
    gx = torch.full((4, 4), 77.0, device=ctx.device)
    arg = torch.full((3, 4), 77, dtype=torch.int32, device=ctx.device)
    run = lambda *a: lb.vgl_hip_agg_run(*a)  # noqa: E731
    back = lambda *a: lb.vgl_hip_agg_run_transposed(*a)  # noqa: E731
    other = A.Context(0)
    refused = [
        run(None, h, 0, None, ptr(x), 4, 4, ptr(out), 4, None, None), run(ctx.h, None, 0, None, ptr(x), 4, 4, ptr(out), 4, None, None),
        run(ctx.h, h, 0, None, None, 4, 4, ptr(out), 4, None, None), run(ctx.h, h, 0, None, ptr(x), 4, 4, None, 4, None, None),
        run(ctx.h, h, 0, None, ptr(x), 4, 0, ptr(out), 4, None, None), run(ctx.h, h, 0, None, ptr(x), 3, 4, ptr(out), 4, None, None),
        run(ctx.h, h, 0, None, ptr(x), 4, 4, ptr(out), 3, None, None), run(ctx.h, h, 4, None, ptr(x), 4, 4, ptr(out), 4, None, None),
        run(ctx.h, h, -1, None, ptr(x), 4, 4, ptr(out), 4, None, None), run(ctx.h, h, 2, ptr(w), ptr(x), 4, 4, ptr(out), 4, ptr(arg), None),
        run(ctx.h, h, 3, ptr(w), ptr(x), 4, 4, ptr(out), 4, None, None), run(other.h, h, 0, None, ptr(x), 4, 4, ptr(out), 4, None, None),
        back(ctx.h, h, 2, None, None, ptr(out), 4, 4, ptr(gx), 4, None), back(ctx.h, h, 3, None, None, ptr(out), 4, 4, ptr(gx), 4, None),
        back(ctx.h, h, 0, None, None, None, 4, 4, ptr(gx), 4, None), back(ctx.h, h, 0, None, None, ptr(out), 4, 4, None, 4, None),
        back(ctx.h, h, 0, None, None, ptr(out), 3, 4, ptr(gx), 4, None), back(ctx.h, h, 0, None, None, ptr(out), 4, 4, ptr(gx), 3, None),
        back(ctx.h, h, 1, None, None, ptr(out), 4, 0, ptr(gx), 4, None), back(ctx.h, h, 7, None, None, ptr(out), 4, 4, ptr(gx), 4, None),
        back(ctx.h, h, 2, ptr(w), ptr(arg), ptr(out), 4, 4, ptr(gx), 4, None), back(other.h, h, 0, None, None, ptr(out), 4, 4, ptr(gx), 4, None),
        lb.vgl_hip_agg_plan_info(None, C.byref(L.AggStats())), lb.vgl_hip_agg_plan_info(h, None),
    ]
    assert all(rc != 0 for rc in refused), refused
    ctx.sync()
    assert (out == 77.0).all() and (gx == 77.0).all() and (arg == 77).all()
    st = L.AggStats()
    assert run(ctx.h, h, 2, None, ptr(x), 4, 4, ptr(out), 4, ptr(arg), C.byref(st)) == 0 and st.rows == 3 and st.entries == 5 and st.vec == 4
    assert np.array_equal(arg.cpu().numpy(), R.forward(rowptr, adj, x.cpu().numpy(), "max")[1])
    assert lb.vgl_hip_agg_plan_destroy(ctx.h, h) == 0 and lb.vgl_hip_agg_plan_destroy(ctx.h, None) == 0 and lb.vgl_hip_agg_plan_destroy(None, None) != 0
    other.close()


def test_empty_shapes(ctx):
    """no rows, no columns, no entries: nothing to walk, outputs of the right shape (0 in empty rows, arg -1)"""
    A = api()
    rowptr = np.zeros(4, dtype=np.int64)
    plan = plan_of(ctx, rowptr, np.zeros(0, dtype=np.int32), 2)
    xt = torch.ones((2, 3), device=ctx.device, requires_grad=True)
    out, arg = A.aggregate(plan, xt, "min", return_arg=True)
    assert out.tolist() == [[0.0] * 3] * 3 and arg.tolist() == [[-1] * 3] * 3
    A.aggregate(plan, xt, "mean").sum().backward()
    assert xt.grad.tolist() == [[0.0] * 3] * 2
    plan.close()
    plan = plan_of(ctx, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 2)
    assert tuple(A.aggregate(plan, torch.ones((2, 3), device=ctx.device)).shape) == (0, 3)
    plan.close()


@pytest.mark.parametrize("extra", [[], ["-backward", "-op", "max"], ["-weighted", "-op", "mean", "-backward", "-features", "12"]])
def test_app_check(extra):
    cmd = [os.path.join(ROOT, "apps", "bin", "agg_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-check"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "AGG launches:" in out.stdout, out.stdout
