"""Heads on the GPU (the five vgl_hip_agg_*_heads calls, api.sddmm(heads=) / edge_softmax on E x H / spmm with E x H weights / graph_attention(heads=),
apps/bin/attn_hip -heads) against the numpy restatement (tests/heads_reference.py) and against the single-head calls.  The contract is equality of
bits: column h of the heads dot product and of the heads softmax IS the single-head call on head h's slice, the heads runs with equal weight columns
ARE the single-head runs, H = 1 IS the single-head call.  As in test_edge_gpu.py the restatement is met on data where every product and partial sum
is exact in float32 (integers in [-8, 8]: the largest partial sum is 64 x 4097 < 2^24), and real-valued data is held to the derived bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import agg_reference as AR
import edge_reference as ER
import heads_reference as HR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHRUNK = {"VGL_AGG_SHORT": "4", "VGL_AGG_WAVE": "16", "VGL_AGG_CHUNK": "64"}
LONG = list(range(67)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
NEG_INF = np.float32(-np.inf)
# (H, D): one head; heads narrower than a vector; D = 16, 8, 4 at 4, 8, 16 heads; (3, 12): three groups per head, one padded lane; (2, 36): a head
# wider than a short team's tile; (2, 260): a head of more than one tile in the wave class; (64, 1): passes in the short class
HEADS = [(1, 8), (2, 1), (2, 3), (2, 4), (2, 5), (4, 16), (8, 8), (16, 4), (3, 12), (2, 36), (2, 260), (64, 1)]
SUM, MEAN, MAX, MIN = 0, 1, 2, 3


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


def check_classes(st, plan, rowptr, **switches):
    for k, v in AR.classify(rowptr, **switches).items():
        assert st[k] == v and plan.info()[k] == v, (k, st[k], v)


# ---- SDDMM with heads: the slice calls bit for bit, the restatement on integers ----
def check_dot(ctx, plan, rowptr, adj, n_cols, H, D, rng, what, **switches):
    A = api()
    F, E = H * D, len(adj)
    a, b = ints(rng, len(rowptr) - 1, F), ints(rng, n_cols, F)
    at, bt = dev(ctx, a), dev(ctx, b)
    e = A.sddmm(plan, at, bt, heads=H)
    st = plan.last_edge_stats
    assert e.dtype == torch.float32 and tuple(e.shape) == (E, H) and e.is_contiguous(), what
    assert np.array_equal(host(e), HR.sddmm(rowptr, adj, a, b, H)[0]), what
    vec = HR.dot_vec(D)
    check_classes(st, plan, rowptr, **switches)
    assert (st["heads"], st["vec"], st["transposed"]) == (H, vec, 0) and st["column_tiles"] == HR.dot_walks(F, H, vec), (what, st)
    assert st["algorithmic_bytes"] == HR.bytes_sddmm(rowptr, F, H, vec, **switches), what
    mean = plan._sddmm_heads(at, bt, H, 1)                              # an exact sum, one correctly rounded division
    assert np.array_equal(host(mean), HR.sddmm(rowptr, adj, a, b, H, mean=True)[0]), what + " mean"
    for h in range(H):
        one = A.sddmm(plan, at[:, h * D:(h + 1) * D], bt[:, h * D:(h + 1) * D])
        assert plan.last_edge_stats["vec"] == vec and plan.last_edge_stats["heads"] == 0, what
        assert same_bits(e[:, h], one), "%s head %d" % (what, h)


@pytest.mark.parametrize("H,D", [(4, 4), (3, 3)])
def test_sddmm_heads_row_lengths_at_the_default_bounds(ctx, H, D):
    rng = np.random.default_rng(1)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check_dot(ctx, plan, rowptr, adj, 97, H, D, rng, "default bounds %dx%d" % (H, D))
    plan.close()


@pytest.mark.parametrize("H,D", [(2, 4), (3, 1), (4, 10)])
def test_sddmm_heads_row_lengths_under_shrunk_bounds(ctx, monkeypatch, H, D):
    switches = shrink(monkeypatch)
    rng = np.random.default_rng(2)
    rowptr, adj = csr_of(list(range(131)), 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check_dot(ctx, plan, rowptr, adj, 11, H, D, rng, "shrunk bounds %dx%d" % (H, D), **switches)
    assert plan.info()["hub_rows"] == 131 - 65
    plan.close()


@pytest.fixture(scope="module")
def three_rows():
    rng = np.random.default_rng(3)
    return csr_of([5, 100, 2000], 50, rng)


@pytest.mark.parametrize("H,D", HEADS)
def test_sddmm_heads_shapes(ctx, three_rows, H, D):
    """a short, a wave and a workgroup row under every lane layout of the list"""
    rowptr, adj = three_rows
    plan = plan_of(ctx, rowptr, adj, 50)
    check_dot(ctx, plan, rowptr, adj, 50, H, D, np.random.default_rng(100 + H * D), "shapes %dx%d" % (H, D))
    plan.close()


def test_sddmm_heads_views(ctx):
    """an offset view that starts one element off 16 bytes takes the scalar path and still equals the slice calls; a column slice goes with its
    leading dimension"""
    A = api()
    rng = np.random.default_rng(4)
    rowptr, adj = csr_of(list(range(67)), 67, rng)
    plan = plan_of(ctx, rowptr, adj, 67)
    H, D = 2, 4
    a, b = ints(rng, 67, 8), ints(rng, 67, 8)
    want = HR.sddmm(rowptr, adj, a, b, H)[0]
    flat = torch.zeros(67 * 8 + 1, dtype=torch.float32, device=ctx.device)
    view = flat[1:].view(67, 8)
    view.copy_(dev(ctx, a))
    e = A.sddmm(plan, view, dev(ctx, b), heads=H)
    assert view.storage_offset() == 1 and np.array_equal(host(e), want) and plan.last_edge_stats["vec"] == 1
    assert plan.last_edge_stats["column_tiles"] == HR.dot_walks(8, 2, 1)
    for h in range(H):
        assert same_bits(e[:, h], A.sddmm(plan, view[:, h * D:(h + 1) * D], dev(ctx, b)[:, h * D:(h + 1) * D])) and plan.last_edge_stats["vec"] == 1
    assert np.array_equal(host(A.sddmm(plan, dev(ctx, a), dev(ctx, b), heads=H)), want) and plan.last_edge_stats["vec"] == 4
    wide = torch.zeros((67, 20), dtype=torch.float32, device=ctx.device)
    for first, vec in ((4, 4), (1, 1)):
        wide.zero_()
        wide[:, first:first + 8] = dev(ctx, b)
        piece = wide[:, first:first + 8]
        assert not piece.is_contiguous() and np.array_equal(host(A.sddmm(plan, dev(ctx, a), piece, heads=H)), want) and plan.last_edge_stats["vec"] == vec
        assert np.array_equal(host(A.sddmm(plan, piece, dev(ctx, a), heads=H)), HR.sddmm(rowptr, adj, b, a, H)[0])
    # the gradients reach the leaves behind slices
    la = torch.zeros((67, 20), dtype=torch.float32, device=ctx.device, requires_grad=True)
    with torch.no_grad():
        la[:, 4:12] = dev(ctx, a)
    ge = ints(rng, len(adj), H)
    A.sddmm(plan, la[:, 4:12], dev(ctx, b), heads=H).backward(dev(ctx, ge))
    ga, _ = HR.sddmm_backward64(rowptr, adj, 67, a, b, ge, H)
    assert np.array_equal(host(la.grad)[:, 4:12], ga.astype(np.float32)) and not host(la.grad)[:, :4].any() and not host(la.grad)[:, 12:].any()
    plan.close()


# ---- edge softmax with heads: the per-column calls bit for bit, exact values ----
def scores(rowptr, H):
    """constant per (row, head), different between heads and between rows"""
    row = row_index(rowptr)
    return (((row[:, None] + 2 * np.arange(H)[None, :]) % 7) - 3).astype(np.float32)


def check_softmax(ctx, plan, rowptr, H, rng, what, **switches):
    A = api()
    row, length = row_index(rowptr), np.diff(rowptr)
    E = int(rowptr[-1])
    e = scores(rowptr, H)
    y = plan._edge_softmax_heads(dev(ctx, e))
    assert tuple(y.shape) == (E, H) and np.array_equal(host(y), np.repeat((np.float32(1) / length[row].astype(np.float32))[:, None], H, axis=1)), what
    assert plan.last_edge_stats["heads"] == H and plan.last_edge_stats["algorithmic_bytes"] == HR.bytes_softmax(rowptr, H, **switches), what
    # a hashed subset at -inf that differs per head; rows fully masked in one head only: row % 3 == h % 3
    dead = (rng.random((E, H)) < 0.4) | ((row[:, None] % 3) == (np.arange(H)[None, :] % 3))
    masked = np.where(dead, NEG_INF, e)
    want = HR.edge_softmax(rowptr, masked)[0]
    live = np.zeros((len(length), H), dtype=np.int64)
    np.add.at(live, row, ~dead)
    with np.errstate(divide="ignore"):
        assert np.array_equal(want, np.where(dead, np.float32(0), np.float32(1) / live[row].astype(np.float32)).astype(np.float32))
    mt = dev(ctx, masked)
    y = plan._edge_softmax_heads(mt)
    assert np.array_equal(host(y), want) and not np.isnan(host(y)).any(), what
    for h in range(H):
        assert same_bits(y[:, h], A.edge_softmax(plan, mt[:, h].contiguous())), "%s head %d" % (what, h)
        assert plan.last_edge_stats["heads"] == 0
    if H > 1:
        assert same_bits(A.edge_softmax(plan, mt), y)


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8, 16])
def test_edge_softmax_heads_exact_at_the_default_bounds(ctx, H):
    rng = np.random.default_rng(6)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check_softmax(ctx, plan, rowptr, H, rng, "default bounds H=%d" % H)
    check_classes(plan.last_edge_stats, plan, rowptr)
    plan.close()


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8, 16])
def test_edge_softmax_heads_exact_under_shrunk_bounds(ctx, monkeypatch, H):
    """lengths 0 .. 130 in chunks of 64, and a row of 190 = 3 chunks whose middle chunk is dead in head 0 only and whose only live entry of head 1
    (where there is one) sits in the last chunk"""
    switches = shrink(monkeypatch)
    rng = np.random.default_rng(7)
    rowptr, adj = csr_of(list(range(131)) + [190], 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check_softmax(ctx, plan, rowptr, H, rng, "shrunk bounds H=%d" % H, **switches)
    e = np.full((int(rowptr[-1]), H), 2.5, dtype=np.float32) + np.arange(H, dtype=np.float32)[None, :]
    lo, hi = int(rowptr[131]), int(rowptr[132])
    e[lo + 64:lo + 128, 0] = NEG_INF
    if H > 1:
        e[lo:hi - 1, 1] = NEG_INF
    y = host(plan._edge_softmax_heads(dev(ctx, e)))[lo:hi]
    assert np.array_equal(y[:64, 0], np.full(64, np.float32(1) / np.float32(126))) and not y[64:128, 0].any() and np.array_equal(y[128:, 0], np.full(62, np.float32(1) / np.float32(126)))
    if H > 1:
        assert not y[:-1, 1].any() and y[-1, 1] == 1.0
    assert np.array_equal(y[:, 2:], np.full((190, max(H - 2, 0)), np.float32(1) / np.float32(190)))
    plan.close()


def check_softmax_backward(ctx, plan, rowptr, H, rng, what, **switches):
    E = int(rowptr[-1])
    y, gy = rng.choice(np.array([0.25, 0.5, 1.0], dtype=np.float32), (E, H)), ints(rng, E, H)
    yt, gt = dev(ctx, y), dev(ctx, gy)
    ge = plan._edge_softmax_backward_heads(yt, gt)                      # the formula on any y: every product and partial sum is exact
    assert plan.last_edge_stats["heads"] == H and plan.last_edge_stats["algorithmic_bytes"] == HR.bytes_softmax(rowptr, H, backward=True, **switches)
    want, exact, _ = HR.edge_softmax_backward(rowptr, y, gy)
    assert np.array_equal(want.astype(np.float64), exact) and np.array_equal(host(ge), want), what
    for h in range(H):
        assert same_bits(ge[:, h], plan._edge_softmax_backward(yt[:, h].contiguous(), gt[:, h].contiguous())), "%s head %d" % (what, h)


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8, 16])
def test_edge_softmax_backward_heads_exact(ctx, monkeypatch, H):
    rng = np.random.default_rng(8)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check_softmax_backward(ctx, plan, rowptr, H, rng, "default bounds H=%d" % H)
    plan.close()
    switches = shrink(monkeypatch)
    rowptr, adj = csr_of(list(range(131)), 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check_softmax_backward(ctx, plan, rowptr, H, rng, "shrunk bounds H=%d" % H, **switches)
    plan.close()


# ---- the two runs with E x H weights ----
def check_runs(ctx, plan, rowptr, adj, n_cols, H, D, rng, what, **switches):
    A = api()
    F, E, n = H * D, len(adj), len(rowptr) - 1
    w, x, g = ints(rng, E, H), ints(rng, n_cols, F), ints(rng, n, F)
    wt, xt, gt = dev(ctx, w), dev(ctx, x), dev(ctx, g)
    vec = HR.dot_vec(D)
    t_rowptr = AR.transpose(rowptr, adj, n_cols)[0]
    for op in ("sum", "mean"):
        out = plan._forward_heads(xt, A.AGG_OPS[op], wt, H)
        st = plan.last_stats
        assert np.array_equal(host(out), HR.run(rowptr, adj, x, op, w)[0]), "%s %s" % (what, op)       # an exact sum; mean: one correctly rounded division
        check_classes(st, plan, rowptr, **switches)
        assert (st["heads"], st["vec"], st["transposed"]) == (H, vec, 0) and st["column_tiles"] == AR.column_tiles(F, vec), (what, st)
        assert st["algorithmic_bytes"] == HR.bytes_run(rowptr, F, H, vec, **switches), what
        gx = plan._backward_heads(gt, A.AGG_OPS[op], wt, H)
        st = plan.last_backward_stats
        want, mag, exact = HR.run_transposed(rowptr, adj, n_cols, g, op, w)
        if op == "sum":
            assert np.array_equal(host(gx), want), what + " transposed"
        else:                                                           # w / len is rounded: the bound
            assert np.all(np.abs(host(gx) - exact) <= AR.tolerance(int(np.diff(t_rowptr).max(initial=0))) * mag), what + " transposed mean"
        assert (st["heads"], st["vec"], st["transposed"], st["rows"]) == (H, vec, 1, n_cols) and st["column_tiles"] == AR.column_tiles(F, vec), (what, st)
        assert st["algorithmic_bytes"] == HR.bytes_run(t_rowptr, F, H, vec, transposed=True, mean=op == "mean", **switches), what


@pytest.mark.parametrize("H,D", [(4, 4), (3, 3)])
def test_runs_heads_row_lengths_at_the_default_bounds(ctx, H, D):
    rng = np.random.default_rng(21)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    check_runs(ctx, plan, rowptr, adj, 97, H, D, rng, "default bounds %dx%d" % (H, D))
    plan.close()


@pytest.mark.parametrize("H,D", [(2, 4), (3, 1), (4, 10)])
def test_runs_heads_row_lengths_under_shrunk_bounds(ctx, monkeypatch, H, D):
    switches = shrink(monkeypatch)
    rng = np.random.default_rng(22)
    rowptr, adj = csr_of(list(range(131)), 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    check_runs(ctx, plan, rowptr, adj, 11, H, D, rng, "shrunk bounds %dx%d" % (H, D), **switches)
    plan.close()


@pytest.mark.parametrize("H,D", HEADS)
def test_runs_heads_shapes(ctx, three_rows, H, D):
    rowptr, adj = three_rows
    plan = plan_of(ctx, rowptr, adj, 50)
    check_runs(ctx, plan, rowptr, adj, 50, H, D, np.random.default_rng(200 + H * D), "shapes %dx%d" % (H, D))
    plan.close()


@pytest.mark.parametrize("H,D", [(4, 4), (3, 3), (2, 8), (5, 1)])
@pytest.mark.parametrize("op", ["sum", "mean"])
def test_runs_heads_with_equal_weight_columns_are_the_single_head_runs(ctx, H, D, op):
    """real-valued data: where both calls pick the same VEC the heads run with H equal weight columns has the bits of the single-head run"""
    A = api()
    rng = np.random.default_rng(23)
    rowptr, adj = csr_of(LONG, 97, rng)
    F, E, n = H * D, len(adj), len(LONG)
    plan = plan_of(ctx, rowptr, adj, 97)
    w, x, g = (dev(ctx, rng.standard_normal(s).astype(np.float32)) for s in ((E,), (97, F), (n, F)))
    wh = w[:, None].repeat(1, H).contiguous()
    vec = HR.dot_vec(D)
    assert vec == HR.dot_vec(F)
    out = plan._forward_heads(x, A.AGG_OPS[op], wh, H)
    assert (plan.last_stats["vec"], plan.last_stats["heads"]) == (vec, H)
    single = plan._forward(x, A.AGG_OPS[op], w)[0]
    assert (plan.last_stats["vec"], plan.last_stats["heads"]) == (vec, 0) and same_bits(out, single)
    gx = plan._backward_heads(g, A.AGG_OPS[op], wh, H)
    assert (plan.last_backward_stats["vec"], plan.last_backward_stats["heads"]) == (vec, H)
    single = plan._backward(g, A.AGG_OPS[op], w, None)
    assert (plan.last_backward_stats["vec"], plan.last_backward_stats["heads"]) == (vec, 0) and same_bits(gx, single)
    plan.close()


def test_runs_heads_on_stars_of_40000_entries(ctx):
    """one row of 40 000 entries (three chunks in the forward run), and 40 000 rows that all list column 0 (three chunks in the transposed run)"""
    rng = np.random.default_rng(24)
    n = 40000
    rowptr = np.zeros(n + 2, dtype=np.int64)
    rowptr[1:] = n
    plan = plan_of(ctx, rowptr, np.arange(1, n + 1, dtype=np.int32), n + 1)
    check_runs(ctx, plan, rowptr, np.arange(1, n + 1, dtype=np.int32), n + 1, 4, 4, rng, "in-star")
    assert (plan.last_stats["chunks"], plan.last_stats["hub_rows"]) == (3, 1)
    check_dot(ctx, plan, rowptr, np.arange(1, n + 1, dtype=np.int32), n + 1, 2, 4, rng, "in-star")
    plan.close()
    rowptr, adj = np.arange(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    plan = plan_of(ctx, rowptr, adj, 3)
    check_runs(ctx, plan, rowptr, adj, 3, 4, 4, rng, "out-star")
    assert (plan.last_backward_stats["chunks"], plan.last_backward_stats["hub_rows"]) == (3, 1)
    plan.close()


# ---- one head is the single-head call; real-valued data ----
def test_one_head_returns_the_bits_of_the_single_head_calls(ctx):
    A = api()
    rng = np.random.default_rng(25)
    lengths = LONG + [40000]
    rowptr, adj = csr_of(lengths, 61, rng)
    E, F, n = len(adj), 8, len(lengths)
    plan = plan_of(ctx, rowptr, adj, 61)
    a, b, g = (dev(ctx, rng.standard_normal(s).astype(np.float32)) for s in ((n, F), (61, F), (n, F)))
    e, gy = dev(ctx, rng.uniform(-8, 8, E).astype(np.float32)), dev(ctx, rng.standard_normal(E).astype(np.float32))
    for mean in (0, 1):
        assert same_bits(plan._sddmm_heads(a, b, 1, mean)[:, 0], plan._sddmm(a, b, mean))
    y = plan._edge_softmax(e)
    assert same_bits(plan._edge_softmax_heads(e[:, None].contiguous())[:, 0], y)
    assert same_bits(plan._edge_softmax_backward_heads(y[:, None].contiguous(), gy[:, None].contiguous())[:, 0], plan._edge_softmax_backward(y, gy))
    for op in (SUM, MEAN):
        assert same_bits(plan._forward_heads(b, op, e[:, None].contiguous(), 1), plan._forward(b, op, e)[0])
        assert same_bits(plan._backward_heads(g, op, e[:, None].contiguous(), 1), plan._backward(g, op, e, None))
    assert same_bits(A.graph_attention(plan, a, b, b, heads=1), A.graph_attention(plan, a, b, b))
    plan.close()


def test_real_valued_inputs_within_the_bounds_and_the_same_bits_twice(ctx):
    A = api()
    rng = np.random.default_rng(11)
    lengths = LONG + [40000]
    rowptr, adj = csr_of(lengths, 61, rng)
    E, H, D, n = len(adj), 4, 8, len(lengths)
    F = H * D
    a, b, g = (rng.uniform(-0.5, 0.5, s).astype(np.float32) for s in ((n, F), (61, F), (n, F)))
    e, gy = rng.uniform(-8, 8, (E, H)).astype(np.float32), rng.standard_normal((E, H)).astype(np.float32)
    plan = plan_of(ctx, rowptr, adj, 61)

    def within(got, exact, bound, what):
        err = np.abs(got.astype(np.float64) - exact)
        print(what, "largest error", float(err.max(initial=0.0)), "largest bound", float(bound.max(initial=0.0)), "largest error / bound",
              float((err / np.maximum(bound, 1e-300)).max(initial=0.0)))
        assert np.all(err <= bound), what

    runs = []
    for _ in range(2):
        dot = A.sddmm(plan, dev(ctx, a), dev(ctx, b), heads=H)
        mean = plan._sddmm_heads(dev(ctx, a), dev(ctx, b), H, 1)
        y = A.edge_softmax(plan, dev(ctx, e))
        ge = plan._edge_softmax_backward_heads(y, dev(ctx, gy))
        out = A.spmm(plan, y, dev(ctx, b))
        gx = plan._backward_heads(dev(ctx, g), MEAN, y, H)
        runs.append((dot, mean, y, ge, out, gx))
    assert all(same_bits(p, q) for p, q in zip(*runs))
    dot, mean, y, ge, out, gx = (host(t) for t in runs[0])
    for got, is_mean in ((dot, False), (mean, True)):
        _, mag, exact = HR.sddmm(rowptr, adj, a, b, H, mean=is_mean)
        within(got, exact, ER.dot_bound(D) * mag, "dot mean=%d" % is_mean)
    _, exact, R, d = HR.edge_softmax(rowptr, e)
    assert R.max() <= 16
    within(y, exact, ER.softmax_bound(d, R) * exact + ER.TINY, "softmax")
    _, gexact, gmag = HR.edge_softmax_backward(rowptr, y, gy)           # y is data: the device's own
    within(ge, gexact, ER.softmax_backward_bound(d) * gmag, "softmax backward")
    _, omag, oexact = HR.run(rowptr, adj, b, "sum", y)
    within(out, oexact, AR.tolerance(40000) * omag, "run")
    _, tmag, texact = HR.run_transposed(rowptr, adj, 61, g, "mean", y)
    within(gx, texact, AR.tolerance(int(np.bincount(adj, minlength=61).max())) * tmag, "run transposed mean")
    plan.close()


# ---- gradient wiring ----
def test_sddmm_heads_gradients_are_the_two_heads_runs(ctx):
    A = api()
    rng = np.random.default_rng(12)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    H = 4
    a, b = rng.standard_normal((len(LONG), 16)).astype(np.float32), rng.standard_normal((97, 16)).astype(np.float32)
    ge = dev(ctx, rng.standard_normal((len(adj), H)).astype(np.float32))
    at, bt = dev(ctx, a).requires_grad_(True), dev(ctx, b).requires_grad_(True)
    A.sddmm(plan, at, bt, heads=H).backward(ge)
    assert same_bits(at.grad, plan._forward_heads(dev(ctx, b), SUM, ge, H))
    assert same_bits(bt.grad, plan._backward_heads(dev(ctx, a), SUM, ge, H))
    only = dev(ctx, a).requires_grad_(True)                              # needs_input_grad: b asks for nothing
    A.sddmm(plan, only, dev(ctx, b), heads=H).backward(ge)
    assert same_bits(only.grad, at.grad)
    with pytest.raises(lib().VglHipError, match="SDDMM"):
        A.aggregate(plan, dev(ctx, b), "sum", ge[:, 0].contiguous().requires_grad_(True))
    plan.close()


@pytest.mark.parametrize("op", ["sum", "mean"])
def test_spmm_and_sddmm_heads_gradients_equal_torch_cpu_autograd_on_integer_data(ctx, op):
    A = api()
    rng = np.random.default_rng(13)
    lengths = [0, 1, 2, 5, 9, 33, 40, 70, 0, 3, 1100]
    rowptr, adj = csr_of(lengths, 17, rng)
    H, D, n, E = 3, 2, len(lengths), int(rowptr[-1])
    w, x, g = rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), (E, H)), ints(rng, 17, 6), ints(rng, n, 6)
    plan = plan_of(ctx, rowptr, adj, 17)
    wt, xt = dev(ctx, w).requires_grad_(True), dev(ctx, x).requires_grad_(True)
    out = A.spmm(plan, wt, xt, op)
    out.backward(dev(ctx, g))
    row, at = torch.as_tensor(row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    wc, xc = torch.tensor(w.astype(np.float64), requires_grad=True), torch.tensor(x.astype(np.float64), requires_grad=True)
    ref = torch.zeros((n, H, D), dtype=torch.float64).index_add_(0, row, wc[:, :, None] * xc[at].view(-1, H, D)).view(n, 6)
    if op == "mean":
        ref = ref / torch.as_tensor(np.maximum(lengths, 1)[:, None].astype(np.float64))
    (ref * torch.as_tensor(g.astype(np.float64))).sum().backward()
    assert np.array_equal(host(out), ref.detach().numpy().astype(np.float32))
    assert tuple(wt.grad.shape) == (E, H) and np.array_equal(host(wt.grad), wc.grad.numpy().astype(np.float32)), "grad weight"     # an integer dot product, one division
    if op == "sum":
        assert np.array_equal(host(xt.grad), xc.grad.numpy().astype(np.float32)), "grad x"
        a, ge = ints(rng, n, 6), ints(rng, E, H)
        ad, bd = dev(ctx, a).requires_grad_(True), dev(ctx, x).requires_grad_(True)
        e = A.sddmm(plan, ad, bd, heads=H)
        e.backward(dev(ctx, ge))
        ac, bc = torch.tensor(a.astype(np.float64), requires_grad=True), torch.tensor(x.astype(np.float64), requires_grad=True)
        ec = (ac[row].view(-1, H, D) * bc[at].view(-1, H, D)).sum(-1)
        (ec * torch.as_tensor(ge.astype(np.float64))).sum().backward()
        assert np.array_equal(host(e), ec.detach().numpy().astype(np.float32))
        assert np.array_equal(host(ad.grad), ac.grad.numpy().astype(np.float32)) and np.array_equal(host(bd.grad), bc.grad.numpy().astype(np.float32))
    else:
        _, gmag, gexact = HR.run_transposed(rowptr, adj, 17, g, "mean", w)
        assert np.all(np.abs(host(xt.grad) - gexact) <= AR.tolerance(int(np.bincount(adj, minlength=17).max())) * gmag), "grad x"
    plan.close()


POWERS = [1, 2, 4, 8, 16, 32, 64, 128, 1024, 2048, 4096, 32768]


def test_edge_softmax_heads_loss_backward_on_rows_of_power_of_two_length(ctx):
    """a constant score per (row, head) gives y = 1 / len, a power of two: the gradient through loss.backward() is exact (32768: two default chunks)"""
    A = api()
    rng = np.random.default_rng(10)
    rowptr, adj = csr_of(POWERS, 5, rng)
    plan = plan_of(ctx, rowptr, adj, 5)
    H = 4
    e = dev(ctx, scores(rowptr, H)).requires_grad_(True)
    gy = ints(rng, len(adj), H)
    y = A.edge_softmax(plan, e)
    (y * dev(ctx, gy)).sum().backward()
    inv = np.repeat((1.0 / np.diff(rowptr)[row_index(rowptr)])[:, None], H, axis=1)
    assert np.array_equal(host(y).astype(np.float64), inv) and np.array_equal(host(e.grad).astype(np.float64), HR.softmax_backward64(rowptr, inv, gy))
    plan.close()


# ---- attention with heads, end to end ----
def test_graph_attention_heads_is_its_three_parts_and_its_single_head_calls(ctx):
    A = api()
    rng = np.random.default_rng(14)
    rowptr, adj = csr_of(LONG, 97, rng)
    plan = plan_of(ctx, rowptr, adj, 97)
    H, D, Dv = 4, 4, 2
    q, k, v = (rng.standard_normal(s).astype(np.float32) * 0.5 for s in ((len(LONG), H * D), (97, H * D), (97, H * Dv)))
    g = dev(ctx, rng.standard_normal((len(LONG), H * Dv)).astype(np.float32))
    grads = []
    for whole in (True, False):
        qt, kt, vt = (dev(ctx, t).requires_grad_(True) for t in (q, k, v))
        if whole:
            out, w = A.graph_attention(plan, qt, kt, vt, return_weights=True, heads=H)
        else:
            w = A.edge_softmax(plan, A.sddmm(plan, qt, kt, heads=H) * (D ** -0.5))
            out = A.spmm(plan, w, vt)
        out.backward(g)
        grads.append((out.detach(), w.detach(), qt.grad, kt.grad, vt.grad))
    assert tuple(grads[0][1].shape) == (len(adj), H) and all(same_bits(p, r) for p, r in zip(*grads))
    qt, kt, vt = (dev(ctx, t) for t in (q, k, v))
    for h in range(H):
        _, w = A.graph_attention(plan, qt[:, h * D:(h + 1) * D], kt[:, h * D:(h + 1) * D], vt[:, h * Dv:(h + 1) * Dv], scale=D ** -0.5, return_weights=True)
        assert same_bits(grads[0][1][:, h], w), h
    half = A.graph_attention(plan, qt, kt, vt, scale=0.5, heads=H)
    assert same_bits(half, A.spmm(plan, A.edge_softmax(plan, A.sddmm(plan, qt, kt, heads=H) * 0.5), vt))
    plan.close()


def test_graph_attention_heads_exact_with_q_zero_on_rows_of_power_of_two_length(ctx, monkeypatch):
    """q = 0: every weight of every head is 1 / len, a power of two, and with integer k, v, g in [-4, 4] every gradient is a sum of dyadic numbers
    whose partial sums are exact in float32 (test_edge_gpu.py has the count of bits): out, grad q, grad k and grad v equal torch CPU float64
    autograd exactly.  Lengths 1 .. 128 = 2^l under the shrunk bounds: every class, 128: two chunks."""
    A = api()
    shrink(monkeypatch)
    rng = np.random.default_rng(15)
    lengths = [1, 2, 4, 8, 16, 32, 64, 128, 0, 128]
    rowptr, adj = csr_of(lengths, 23, rng)
    n, H, D, Dv = len(lengths), 2, 4, 3
    k, v, g = (rng.integers(-4, 5, s).astype(np.float32) for s in ((23, H * D), (23, H * Dv), (n, H * Dv)))
    plan = plan_of(ctx, rowptr, adj, 23)
    qt, kt, vt = torch.zeros((n, H * D), device=ctx.device, requires_grad=True), dev(ctx, k).requires_grad_(True), dev(ctx, v).requires_grad_(True)
    out = A.graph_attention(plan, qt, kt, vt, heads=H)
    out.backward(dev(ctx, g))
    qc, kc, vc = torch.zeros((n, H * D), dtype=torch.float64, requires_grad=True), torch.tensor(k.astype(np.float64), requires_grad=True), torch.tensor(v.astype(np.float64), requires_grad=True)
    row, a = torch.as_tensor(row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    e = (qc[row].view(-1, H, D) * kc[a].view(-1, H, D)).sum(-1) * 0.5
    w = torch.cat([torch.softmax(e[rowptr[i]:rowptr[i + 1]], 0) for i in range(n)])
    ref = torch.zeros((n, H, Dv), dtype=torch.float64).index_add_(0, row, w[:, :, None] * vc[a].view(-1, H, Dv)).view(n, H * Dv)
    (ref * torch.as_tensor(g.astype(np.float64))).sum().backward()
    for got, want, what in ((out, ref.detach(), "out"), (qt.grad, qc.grad, "grad q"), (kt.grad, kc.grad, "grad k"), (vt.grad, vc.grad, "grad v")):
        assert np.array_equal(host(got).astype(np.float64), want.numpy()), what
    assert qc.grad.abs().sum() > 0 and vc.grad.abs().sum() > 0
    plan.close()


def test_sampled_blocks_two_layer_attention_chain_with_four_heads(ctx):
    """sample_blocks on RMAT-10 x 8, two hops, from_block; each layer attends with 4 heads from a block's seeds over its sampled entries; forward, layer
    by layer, within the bound composed in edge_reference.attention per head (the input of a layer is data: the device's own)"""
    A = api()
    rng = np.random.default_rng(16)
    src, dst = ctx.gen_rmat(10, 8, 5)
    g = A.Graph.from_coo(ctx, 1 << 10, src, dst)
    seeds = torch.tensor(rng.choice(1 << 10, 64, replace=False).astype(np.int32), device=ctx.device)
    blocks = A.sample_blocks(g, seeds, [6, 4], seed=11, direction="in")
    (p0, cols0), (p1, cols1) = A.AggregationPlan.from_block(ctx, blocks[0]), A.AggregationPlan.from_block(ctx, blocks[1])
    F, H = 16, 4
    x = dev(ctx, (rng.standard_normal((p1.n_cols, F)) * 0.5).astype(np.float32))
    at1, at0 = torch.searchsorted(cols1, blocks[1]["seeds"]).long(), torch.searchsorted(cols0, blocks[0]["seeds"]).long()
    h1 = A.graph_attention(p1, x[at1], x, x, heads=H)
    h0 = A.graph_attention(p0, h1[at0], h1, h1, heads=H)
    assert tuple(h1.shape) == (cols0.numel(), F) and tuple(h0.shape) == (64, F)
    for p, q, kv, got, what in ((p1, x[at1], x, h1, "layer 1"), (p0, h1[at0], h1, h0, "layer 0")):
        r = HR.attention(host(p.rowptr), host(p.adj), host(q), host(kv), host(kv), H)
        err = np.abs(host(got).astype(np.float64) - r["out"])
        print(what, "largest error", float(err.max()), "largest bound", float(r["bound"].max()))
        assert np.all(err <= r["bound"]), what
    p0.close(); p1.close(); g.close()


# ---- stats, refusals, housekeeping ----
def test_c_refusals_come_before_any_write_and_the_stats_term_by_term(ctx):
    A, L = api(), lib()
    lb = ctx.L
    rng = np.random.default_rng(19)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    h = plan.h
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    a, b = dev(ctx, ints(rng, 3, 4)), dev(ctx, ints(rng, 4, 4))
    e, y, ge = (torch.full((5, 2), 77.0, device=ctx.device) for _ in range(3))
    out, gx = torch.full((3, 4), 77.0, device=ctx.device), torch.full((4, 4), 77.0, device=ctx.device)
    other = A.Context(0)
    dot, sm, back = lb.vgl_hip_agg_sddmm_heads, lb.vgl_hip_agg_edge_softmax_heads, lb.vgl_hip_agg_edge_softmax_backward_heads
    run, tr = lb.vgl_hip_agg_run_heads, lb.vgl_hip_agg_run_transposed_heads
    refused = [
        dot(None, h, ptr(a), 4, ptr(b), 4, 4, 2, 0, ptr(e), None), dot(ctx.h, None, ptr(a), 4, ptr(b), 4, 4, 2, 0, ptr(e), None),
        dot(ctx.h, h, None, 4, ptr(b), 4, 4, 2, 0, ptr(e), None), dot(ctx.h, h, ptr(a), 4, None, 4, 4, 2, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 2, 0, None, None), dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 0, 2, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 0, 0, ptr(e), None), dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, -2, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 3, 0, ptr(e), None), dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 8, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 3, ptr(b), 4, 4, 2, 0, ptr(e), None), dot(ctx.h, h, ptr(a), 4, ptr(b), 3, 4, 2, 0, ptr(e), None),
        dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 2, 2, ptr(e), None), dot(other.h, h, ptr(a), 4, ptr(b), 4, 4, 2, 0, ptr(e), None),
        sm(None, h, ptr(ge), 2, ptr(y), None), sm(ctx.h, None, ptr(ge), 2, ptr(y), None), sm(ctx.h, h, None, 2, ptr(y), None), sm(ctx.h, h, ptr(ge), 2, None, None),
        sm(ctx.h, h, ptr(ge), 0, ptr(y), None), sm(ctx.h, h, ptr(ge), -1, ptr(y), None), sm(other.h, h, ptr(ge), 2, ptr(y), None),
        back(None, h, ptr(y), ptr(e), 2, ptr(ge), None), back(ctx.h, None, ptr(y), ptr(e), 2, ptr(ge), None), back(ctx.h, h, None, ptr(e), 2, ptr(ge), None),
        back(ctx.h, h, ptr(y), None, 2, ptr(ge), None), back(ctx.h, h, ptr(y), ptr(e), 2, None, None), back(ctx.h, h, ptr(y), ptr(e), 0, ptr(ge), None),
        back(other.h, h, ptr(y), ptr(e), 2, ptr(ge), None),
    ]
    for call, x, res in ((run, b, out), (tr, a, gx)):
        refused += [
            call(None, h, SUM, ptr(e), 2, ptr(x), 4, 4, ptr(res), 4, None), call(ctx.h, None, SUM, ptr(e), 2, ptr(x), 4, 4, ptr(res), 4, None),
            call(ctx.h, h, SUM, None, 2, ptr(x), 4, 4, ptr(res), 4, None), call(ctx.h, h, SUM, ptr(e), 2, None, 4, 4, ptr(res), 4, None),
            call(ctx.h, h, SUM, ptr(e), 2, ptr(x), 4, 4, None, 4, None), call(ctx.h, h, SUM, ptr(e), 0, ptr(x), 4, 4, ptr(res), 4, None),
            call(ctx.h, h, SUM, ptr(e), -1, ptr(x), 4, 4, ptr(res), 4, None), call(ctx.h, h, SUM, ptr(e), 3, ptr(x), 4, 4, ptr(res), 4, None),
            call(ctx.h, h, MAX, ptr(e), 2, ptr(x), 4, 4, ptr(res), 4, None), call(ctx.h, h, MIN, ptr(e), 2, ptr(x), 4, 4, ptr(res), 4, None),
            call(ctx.h, h, 4, ptr(e), 2, ptr(x), 4, 4, ptr(res), 4, None), call(ctx.h, h, SUM, ptr(e), 2, ptr(x), 4, 0, ptr(res), 4, None),
            call(ctx.h, h, SUM, ptr(e), 2, ptr(x), 3, 4, ptr(res), 4, None), call(ctx.h, h, SUM, ptr(e), 2, ptr(x), 4, 4, ptr(res), 3, None),
            call(other.h, h, SUM, ptr(e), 2, ptr(x), 4, 4, ptr(res), 4, None),
        ]
    assert all(rc != 0 for rc in refused), refused
    assert b"another context" in lb.vgl_hip_last_error()
    ctx.sync()
    assert all(bool((t == 77.0).all()) for t in (e, y, ge, out, gx))
    assert plan.info()["transposed"] == 0                               # a refused transposed run builds nothing
    st = L.AggStats()
    assert dot(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 2, 0, ptr(e), C.byref(st)) == 0 and (st.rows, st.entries, st.vec, st.transposed, st.heads) == (3, 5, 1, 0, 2)
    assert np.array_equal(host(e), HR.sddmm(rowptr, adj, host(a), host(b), 2)[0]) and list(st.column_tiles) == [1, 1, 1]
    # the models, term by term: the adjacency per walk, what is gathered and written per entry, the bounds and the row per row, the list entries
    assert st.algorithmic_bytes == 5 * 4 + 5 * (4 * 4 + 4 * 2) + 3 * (8 + 4 * 4) + 3 * 4
    assert sm(ctx.h, h, ptr(e), 2, ptr(y), C.byref(st)) == 0 and st.algorithmic_bytes == 5 * 2 * (4 * 3 + 4) + 3 * 8 + 3 * 4 and list(st.column_tiles) == [1, 1, 1] and st.heads == 2
    assert back(ctx.h, h, ptr(y), ptr(e), 2, ptr(ge), C.byref(st)) == 0 and st.algorithmic_bytes == 5 * 2 * (8 * 2 + 4) + 3 * 8 + 3 * 4 and st.heads == 2
    assert run(ctx.h, h, SUM, ptr(e), 2, ptr(b), 4, 4, ptr(out), 4, C.byref(st)) == 0 and (st.heads, st.vec, st.transposed, st.rows) == (2, 1, 0, 3)
    assert st.algorithmic_bytes == 5 * (4 + 4 * 2) + 5 * 4 * 4 + 3 * (8 + 4 * 4) + 3 * 4
    assert tr(ctx.h, h, MEAN, ptr(e), 2, ptr(a), 4, 4, ptr(gx), 4, C.byref(st)) == 0 and (st.heads, st.vec, st.transposed, st.rows) == (2, 1, 1, 4)
    assert st.algorithmic_bytes == 5 * (4 + 4 * 2 + 4 + 16) + 5 * 4 * 4 + 4 * (8 + 4 * 4) + 4 * 4
    # the single-head calls leave heads 0
    one, two = torch.zeros(5, device=ctx.device), torch.zeros(5, device=ctx.device)
    assert lb.vgl_hip_agg_sddmm(ctx.h, h, ptr(a), 4, ptr(b), 4, 4, 0, ptr(one), C.byref(st)) == 0 and st.heads == 0
    assert lb.vgl_hip_agg_edge_softmax(ctx.h, h, ptr(one), ptr(two), C.byref(st)) == 0 and st.heads == 0
    assert lb.vgl_hip_agg_run(ctx.h, h, SUM, ptr(one), ptr(b), 4, 4, ptr(out), 4, None, C.byref(st)) == 0 and st.heads == 0
    assert lb.vgl_hip_agg_run_transposed(ctx.h, h, SUM, ptr(one), None, ptr(a), 4, 4, ptr(gx), 4, C.byref(st)) == 0 and st.heads == 0
    assert plan.info()["heads"] == 0
    other.close()
    plan.close()


def test_python_refusals(ctx):
    A, L = api(), lib()
    rng = np.random.default_rng(18)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    a, b, e = dev(ctx, ints(rng, 3, 4)), dev(ctx, ints(rng, 4, 4)), dev(ctx, ints(rng, 5, 2))
    for bad, match in ((lambda: A.sddmm(plan, a, b, heads=0), "heads must be an int"), (lambda: A.sddmm(plan, a, b, heads=-2), "heads must be an int"),
                       (lambda: A.sddmm(plan, a, b, heads=2.0), "heads must be an int"), (lambda: A.sddmm(plan, a, b, heads=True), "heads must be an int"),
                       (lambda: A.sddmm(plan, a, b, heads=3), "divisible by heads"), (lambda: A.sddmm(plan, a, b[:, :2], heads=2), "same width"),
                       (lambda: A.sddmm(plan, a.double(), b, heads=2), "float64"), (lambda: A.sddmm(plan, a[:2], b, heads=2), "n_rows x F"),
                       (lambda: A.edge_softmax(plan, e.double()), "float64"), (lambda: A.edge_softmax(plan, e[:4]), "per entry"),
                       (lambda: A.edge_softmax(plan, e.cpu()), "per entry"), (lambda: A.edge_softmax(plan, e[:, :1]), "one value per entry"),
                       (lambda: A.edge_softmax(plan, e[:, None, :]), "one value per entry"), (lambda: A.edge_softmax(plan, e[:, :0]), "per entry"),
                       (lambda: A.spmm(plan, e, b, "max"), "'sum' or 'mean'"), (lambda: A.spmm(plan, e.int(), b), "int32"),
                       (lambda: A.spmm(plan, e[:4], b), "per entry"), (lambda: A.spmm(plan, e, b[:, :3]), "divisible by the heads"),
                       (lambda: A.spmm(plan, e, b[:3]), "n_cols x F"), (lambda: A.graph_attention(plan, a, b, b, heads=3), "divisible by heads"),
                       (lambda: A.graph_attention(plan, a, b, b[:, :3], heads=2), "of v must be divisible"),
                       (lambda: A.graph_attention(plan, a, b, b[:3], heads=2), "n_cols x F"), (lambda: A.graph_attention(plan, a, b, b, heads="2"), "heads must be an int"),
                       (lambda: A.aggregate(plan, b, "sum", e), "one value per entry")):
        with pytest.raises(L.VglHipError, match=match):
            bad()
    plan.close()
    for bad in (lambda: A.sddmm(plan, a, b, heads=2), lambda: A.edge_softmax(plan, e), lambda: A.spmm(plan, e, b), lambda: A.graph_attention(plan, a, b, b, heads=2)):
        with pytest.raises(L.VglHipError, match="open AggregationPlan"):
            bad()


def test_empty_shapes(ctx):
    """no entries, no rows, no columns of features: empty or zero tensors of the right shape, and gradients of the right shape"""
    A = api()
    plan = plan_of(ctx, np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), 2)
    q, k = torch.ones((3, 4), device=ctx.device, requires_grad=True), torch.ones((2, 4), device=ctx.device, requires_grad=True)
    e = A.sddmm(plan, q, k, heads=2)
    assert tuple(e.shape) == (0, 2) and tuple(A.edge_softmax(plan, e).shape) == (0, 2)
    out = A.graph_attention(plan, q, k, k, heads=2)
    assert out.tolist() == [[0.0] * 4] * 3
    out.sum().backward()
    assert q.grad.tolist() == [[0.0] * 4] * 3 and k.grad.tolist() == [[0.0] * 4] * 2
    plan.close()
    plan = plan_of(ctx, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 2)
    assert tuple(A.graph_attention(plan, torch.ones((0, 4), device=ctx.device), torch.ones((2, 4), device=ctx.device), torch.ones((2, 4), device=ctx.device), heads=2).shape) == (0, 4)
    plan.close()
    rng = np.random.default_rng(20)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    e = A.sddmm(plan, torch.ones((3, 0), device=ctx.device), torch.ones((4, 0), device=ctx.device), heads=2)
    assert e.tolist() == [[0.0, 0.0]] * 5
    assert tuple(A.spmm(plan, torch.ones((5, 2), device=ctx.device), torch.ones((4, 0), device=ctx.device)).shape) == (3, 0)
    plan.close()


def test_plan_run_destroy_three_times(ctx):
    A = api()
    rng = np.random.default_rng(17)
    rowptr, adj = csr_of(LONG, 97, rng)
    q, k, v = (rng.standard_normal(s).astype(np.float32) * 0.5 for s in ((len(LONG), 8), (97, 8), (97, 8)))
    seen = []
    for _ in range(3):
        plan = plan_of(ctx, rowptr, adj, 97)
        qt = dev(ctx, q).requires_grad_(True)
        out, w = A.graph_attention(plan, qt, dev(ctx, k), dev(ctx, v), return_weights=True, heads=4)
        out.sum().backward()
        seen.append((out.detach().clone(), w.detach().clone(), qt.grad.clone()))
        plan.close()
        assert plan.h is None
    for other in seen[1:]:
        assert all(same_bits(a, b) for a, b in zip(seen[0], other))


@pytest.mark.parametrize("extra", [[], ["-backward", "-features", "12"]])
def test_app_check_with_four_heads(extra):
    cmd = [os.path.join(ROOT, "apps", "bin", "attn_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-heads", "4", "-check"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "heads 4" in out.stdout, out.stdout
    bad = subprocess.run(cmd[:-1 - len(extra)] + ["-features", "10"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0, bad.stdout
