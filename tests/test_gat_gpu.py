"""The additive score of GAT and the entry sums on the GPU (vgl_hip_agg_edge_add_heads / _edge_sum_heads, api.u_add_v / edge_sum / gat_attention,
apps/bin/attn_hip -score add) against the numpy restatement (tests/gat_reference.py).  The score has two roundings and no sum: it is held to
equality of bits.  The sums are met on integers in [-8, 8] with slope 0.25, where every term and every partial sum is exact in float32 (the largest
is 8 x 40 000 < 2^24 and a multiple of 2^-2), so every shape gives the restatement's bits; real-valued data is held to the derived bound
gamma_d * sum |c| and to the same bits on a second run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import agg_reference as AR
import edge_reference as ER
import gat_reference as GR
import heads_reference as HR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHRUNK = {"VGL_AGG_SHORT": "4", "VGL_AGG_WAVE": "16", "VGL_AGG_CHUNK": "64"}
LONG = list(range(67)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
HEADS = [1, 2, 3, 4, 5, 8, 16, 64]
SLOPES = [1.0, 0.2, 0.0]
N_COLS = 97


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


def transposed_csr(rowptr, adj, n_cols):
    """the CSR whose rows are the columns: a plan on it walks, transposed, rows of the lengths of `rowptr`"""
    t_rowptr, t_row, _ = AR.transpose(rowptr, adj, n_cols)
    return t_rowptr, t_row.astype(np.int32)


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_classes(st, walked_rowptr, **switches):
    for k, v in AR.classify(walked_rowptr, **switches).items():
        assert st[k] == v, (k, st[k], v)


@pytest.fixture(scope="module")
def long_csr():
    """every row length of LONG over 97 columns, and its transpose (97 rows that list the rows): left unchanged by the tests"""
    rowptr, adj = csr_of(LONG, N_COLS, np.random.default_rng(1))
    return rowptr, adj, transposed_csr(rowptr, adj, N_COLS)


# ---- the score: bit equality on every class, switch setting and alignment ----
def signed_zeros(rng, *shape):
    return rng.choice(np.array([0.0, -0.0, 1.5, -1.5], dtype=np.float32), shape)


def check_score(ctx, plan, rowptr, adj, H, rng, what, **switches):
    A = api()
    n = len(rowptr) - 1
    for make in (lambda *s: rng.standard_normal(s).astype(np.float32), lambda *s: signed_zeros(rng, *s)):
        s, t = make(n, H), make(N_COLS, H)
        st_, tt = dev(ctx, s), dev(ctx, t)
        for slope in SLOPES:
            e = plan._edge_add(st_, tt, H, slope)
            st = plan.last_edge_stats
            assert e.dtype == torch.float32 and tuple(e.shape) == (len(adj), H) and e.is_contiguous(), what
            assert np.array_equal(bits(host(e)), bits(GR.score(rowptr, adj, s, t, slope))), (what, slope)
            check_classes(st, rowptr, **switches)
            assert (st["heads"], st["vec"], st["transposed"], st["column_tiles"]) == (H, GR.vec_of(H), 0, [1, 1, 1]), (what, st)
            assert st["algorithmic_bytes"] == GR.bytes_score(rowptr, H, **switches), what
            only_s, only_t = plan._edge_add(st_, None, H, slope), plan._edge_add(None, tt, H, slope)
            assert plan.last_edge_stats["algorithmic_bytes"] == GR.bytes_score(rowptr, H, has_s=False, **switches), what
            assert np.array_equal(bits(host(only_s)), bits(GR.score(rowptr, adj, s, None, slope))), (what, slope, "t absent")
            assert np.array_equal(bits(host(only_t)), bits(GR.score(rowptr, adj, None, t, slope))), (what, slope, "s absent")
        assert same_bits(A.u_add_v(plan, st_, tt), plan._edge_add(st_, tt, H, 1.0)) and same_bits(A.u_add_v(plan, st_, tt, 0.2), plan._edge_add(st_, tt, H, 0.2))


@pytest.mark.parametrize("H", HEADS)
def test_score_row_lengths_at_the_default_bounds(ctx, long_csr, H):
    rowptr, adj, _ = long_csr
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    check_score(ctx, plan, rowptr, adj, H, np.random.default_rng(10 + H), "default bounds H=%d" % H)
    plan.close()


@pytest.mark.parametrize("H", HEADS)
def test_score_row_lengths_under_shrunk_bounds(ctx, monkeypatch, long_csr, H):
    switches = shrink(monkeypatch)
    rowptr, adj, _ = long_csr
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    assert plan.info()["hub_rows"] == sum(1 for d in LONG if d > 64)
    check_score(ctx, plan, rowptr, adj, H, np.random.default_rng(30 + H), "shrunk bounds H=%d" % H, **switches)
    plan.close()


@pytest.mark.parametrize("H", [1, 2, 4, 8, 12])
def test_score_views_and_leading_dimensions(ctx, long_csr, H):
    """column slices of a wider matrix go with their leading dimension; a slice or an offset view that leaves 16-byte alignment takes the scalar path
    (vec 1) and gives the same bits"""
    A = api()
    rng = np.random.default_rng(50 + H)
    rowptr, adj, _ = long_csr
    n = len(rowptr) - 1
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    s, t = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((N_COLS, H)).astype(np.float32)
    want = bits(GR.score(rowptr, adj, s, t, 0.2))
    for first, aligned in ((4, True), (1, False), (2, False)):
        ws, wt = torch.zeros((n, H + 8), device=ctx.device), torch.zeros((N_COLS, H + 8), device=ctx.device)
        ws[:, first:first + H], wt[:, first:first + H] = dev(ctx, s), dev(ctx, t)
        ps, pt = ws[:, first:first + H], wt[:, first:first + H]
        assert not ps.is_contiguous() and ps.stride(0) == H + 8
        e = A.u_add_v(plan, ps, pt, 0.2)
        assert np.array_equal(bits(host(e)), want), (H, first)
        # a block of two heads moves in 8-byte pieces at best: vec stays 1; 16-byte pieces need the block of 4 or 8 and the alignment of every array
        assert plan.last_edge_stats["vec"] == (GR.vec_of(H) if aligned and (H + 8) % 4 == 0 else 1), (H, first, plan.last_edge_stats)
        # one side aligned, the other not: still the bits, and vec 1
        assert np.array_equal(bits(host(A.u_add_v(plan, dev(ctx, s), pt, 0.2))), want)
        assert plan.last_edge_stats["vec"] == (GR.vec_of(H) if aligned and (H + 8) % 4 == 0 else 1)
    flat = torch.zeros(n * H + 1, device=ctx.device)
    view = flat[1:].view(n, H)
    view.copy_(dev(ctx, s))
    e = A.u_add_v(plan, view, dev(ctx, t), 0.2)
    assert view.storage_offset() == 1 and np.array_equal(bits(host(e)), want) and plan.last_edge_stats["vec"] == 1
    e = A.u_add_v(plan, dev(ctx, s), dev(ctx, t), 0.2)
    assert np.array_equal(bits(host(e)), want) and plan.last_edge_stats["vec"] == GR.vec_of(H)
    # an E x H output that starts off 16 bytes: the C call on a view
    eflat = torch.zeros(len(adj) * H + 1, device=ctx.device)
    stt = lib().AggStats()
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    sd, td = dev(ctx, s), dev(ctx, t)
    assert ctx.L.vgl_hip_agg_edge_add_heads(ctx.h, plan.h, ptr(sd), H, ptr(td), H, H, 0.2, ptr(eflat[1:]), C.byref(stt)) == 0
    assert stt.vec == 1 and np.array_equal(bits(host(eflat[1:]).reshape(-1, H)), want) and float(eflat[0]) == 0.0
    # one-dimensional terms are one head with (E,) scores
    if H == 1:
        e1 = A.u_add_v(plan, dev(ctx, s[:, 0]), dev(ctx, t[:, 0]), 0.2)
        assert tuple(e1.shape) == (len(adj),) and np.array_equal(bits(host(e1)), want[:, 0])
        wide = torch.zeros((n, 3), device=ctx.device)
        wide[:, 1] = dev(ctx, s[:, 0])
        assert np.array_equal(bits(host(A.u_add_v(plan, wide[:, 1], dev(ctx, t[:, 0]), 0.2))), want[:, 0])          # a strided vector: lds = 3
    plan.close()


# ---- the sums on integers: every shape gives the restatement's bits ----
def gates(rng, E, H):
    g = ints(rng, E, H)                                                # about 1 in 17 is 0: a gate at 0 takes the slope
    g[:, 1::2] *= np.where(g[:, :1] == 0, 1, np.sign(g[:, :1])).astype(np.float32) * -1      # the odd heads flip with the sign of head 0
    return g


def check_sums(ctx, plan, rowptr, adj, n_cols, t_rowptr, H, rng, what, **switches):
    E = len(adj)
    w, gate = ints(rng, E, H), gates(rng, E, H)
    wt, gt = dev(ctx, w), dev(ctx, gate)
    for transposed, walked, rows in ((False, rowptr, len(rowptr) - 1), (True, t_rowptr, n_cols)):
        for g, gd in ((None, None), (gate, gt)):
            out = plan._edge_sum(wt, gd, 0.25, transposed)
            st = plan.last_edge_stats
            want = GR.edge_sum(rowptr, adj, n_cols, w, gate=g, slope=0.25, transposed=transposed)
            assert tuple(out.shape) == (rows, H) and np.array_equal(want[0].astype(np.float64), want[2]), what
            assert np.array_equal(host(out), want[0]), (what, transposed, g is not None)
            check_classes(st, walked, **switches)
            assert (st["heads"], st["vec"], st["transposed"], st["column_tiles"]) == (H, GR.vec_of(H), int(transposed), [1, 1, 1]), (what, st)
            assert st["algorithmic_bytes"] == GR.bytes_sum(walked, H, gate=g is not None, transposed=transposed, **switches), what
    assert plan.info()["transposed"] == 1


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8, 16])
def test_sums_row_and_column_lengths_at_the_default_bounds(ctx, long_csr, H):
    """the plan on the CSR walks LONG forward, the plan on its transpose walks LONG transposed"""
    rowptr, adj, (t_rowptr, t_adj) = long_csr
    rng = np.random.default_rng(70 + H)
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    check_sums(ctx, plan, rowptr, adj, N_COLS, t_rowptr, H, rng, "rows H=%d" % H)
    plan.close()
    plan = plan_of(ctx, t_rowptr, t_adj, len(LONG))
    assert np.array_equal(AR.transpose(t_rowptr, t_adj, len(LONG))[0], rowptr)
    check_sums(ctx, plan, t_rowptr, t_adj, len(LONG), rowptr, H, rng, "columns H=%d" % H)
    plan.close()


@pytest.mark.parametrize("H", [1, 2, 3, 4, 8, 16])
def test_sums_row_and_column_lengths_under_shrunk_bounds(ctx, monkeypatch, long_csr, H):
    switches = shrink(monkeypatch)
    rowptr, adj, (t_rowptr, t_adj) = long_csr
    rng = np.random.default_rng(90 + H)
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    check_sums(ctx, plan, rowptr, adj, N_COLS, t_rowptr, H, rng, "shrunk rows H=%d" % H, **switches)
    plan.close()
    plan = plan_of(ctx, t_rowptr, t_adj, len(LONG))
    check_sums(ctx, plan, t_rowptr, t_adj, len(LONG), rowptr, H, rng, "shrunk columns H=%d" % H, **switches)
    plan.close()


def test_sums_gate_whose_sign_differs_between_heads(ctx, long_csr):
    rowptr, adj, _ = long_csr
    rng = np.random.default_rng(7)
    E, H = len(adj), 4
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    w = ints(rng, E, H)
    gate = np.tile(np.array([1.0, -1.0, 0.0, 2.0], dtype=np.float32), (E, 1))       # open, gated, gated (0 takes the slope), open
    for transposed in (False, True):
        out = host(plan._edge_sum(dev(ctx, w), dev(ctx, gate), 0.25, transposed))
        plain = host(plan._edge_sum(dev(ctx, w), None, 0.25, transposed))
        assert np.array_equal(out[:, [0, 3]], plain[:, [0, 3]]) and np.array_equal(out[:, [1, 2]], np.float32(0.25) * plain[:, [1, 2]])
        assert np.array_equal(out, GR.edge_sum(rowptr, adj, N_COLS, w, gate=gate, slope=0.25, transposed=transposed)[0])
    plan.close()


def test_sums_a_row_and_a_column_of_40000_entries(ctx):
    """three chunks at the default bounds (16384): the partials of the chunks and the hub merge, forward and transposed"""
    rng = np.random.default_rng(8)
    lengths = [40000, 5, 0, 7]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    adj = np.concatenate([np.arange(40000), rng.integers(0, 50000, 12)]).astype(np.int32)      # row 0 lists 40 000 columns once each
    H = 3
    for rp, ad, n_cols, tr_rp, what in ((rowptr, adj, 50000, None, "row"), transposed_csr(rowptr, adj, 50000) + (4, rowptr, "column")):
        plan = plan_of(ctx, rp, ad, n_cols)
        w, gate = ints(rng, len(ad), H), gates(rng, len(ad), H)
        for transposed in (False, True):
            out = plan._edge_sum(dev(ctx, w), dev(ctx, gate), 0.25, transposed)
            assert np.array_equal(host(out), GR.edge_sum(rp, ad, n_cols, w, gate=gate, slope=0.25, transposed=transposed)[0]), (what, transposed)
            if (what == "row") != transposed:
                assert (plan.last_edge_stats["hub_rows"], plan.last_edge_stats["chunks"]) == (1, 3), what
        s, t = ints(rng, len(rp) - 1, H), ints(rng, n_cols, H)
        assert np.array_equal(bits(host(plan._edge_add(dev(ctx, s), dev(ctx, t), H, 0.25))), bits(GR.score(rp, ad, s, t, 0.25))), what
        plan.close()


def test_sums_three_chunks_whose_middle_chunk_is_all_gated(ctx, monkeypatch):
    switches = shrink(monkeypatch)
    rng = np.random.default_rng(9)
    rowptr, adj = csr_of([192, 3, 0, 130], 11, rng)
    plan = plan_of(ctx, rowptr, adj, 11)
    assert AR.classify(rowptr, **switches)["chunks"] == 3 + 3 and plan.info()["hub_rows"] == 2
    H = 2
    w = ints(rng, len(adj), H)
    gate = np.ones((len(adj), H), dtype=np.float32)
    gate[64:128] = -3.0                                                # the second chunk of row 0, every head
    out = host(plan._edge_sum(dev(ctx, w), dev(ctx, gate), 0.25, False))
    want = w[:64].sum(0) + np.float32(0.25) * w[64:128].sum(0) + w[128:192].sum(0)
    assert np.array_equal(out[0], want) and np.array_equal(out, GR.edge_sum(rowptr, adj, 11, w, gate=gate, slope=0.25)[0]) and not out[2].any()
    plan.close()


def test_sums_empty_rows_and_columns_give_zero(ctx):
    rowptr = np.array([0, 2, 2, 5, 5], dtype=np.int64)
    adj = np.array([1, 4, 4, 1, 1], dtype=np.int32)                    # columns 0, 2, 3, 5 are never listed
    plan = plan_of(ctx, rowptr, adj, 6)
    w = dev(ctx, np.arange(1, 11, dtype=np.float32).reshape(5, 2))
    for gate in (None, w):
        rows, cols = torch.full((4, 2), 77.0, device=ctx.device), torch.full((6, 2), 77.0, device=ctx.device)
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
        assert ctx.L.vgl_hip_agg_edge_sum_heads(ctx.h, plan.h, ptr(w), ptr(gate), 0.25, 2, 0, ptr(rows), 2, None) == 0
        assert ctx.L.vgl_hip_agg_edge_sum_heads(ctx.h, plan.h, ptr(w), ptr(gate), 0.25, 2, 1, ptr(cols), 2, None) == 0
        assert rows.tolist() == [[4.0, 6.0], [0.0, 0.0], [21.0, 24.0], [0.0, 0.0]]
        assert cols.tolist() == [[0.0, 0.0], [17.0, 20.0], [0.0, 0.0], [0.0, 0.0], [8.0, 10.0], [0.0, 0.0]]
    plan.close()


# ---- real-valued data: the derived bound on every value, the same bits twice ----
@pytest.mark.parametrize("shrunk", [False, True])
def test_sums_real_valued_within_the_bound_and_the_same_bits_twice(ctx, monkeypatch, long_csr, shrunk):
    if shrunk:
        shrink(monkeypatch)
    rowptr, adj, (t_rowptr, t_adj) = long_csr
    rng = np.random.default_rng(11)
    worst = 0.0
    for rp, ad, n_cols in ((rowptr, adj, N_COLS), (t_rowptr, t_adj, len(LONG))):
        plan = plan_of(ctx, rp, ad, n_cols)
        for H in (1, 4, 5):
            w, gate = rng.standard_normal((len(ad), H)).astype(np.float32), rng.standard_normal((len(ad), H)).astype(np.float32)
            for transposed in (False, True):
                for g in (None, gate):
                    gd = None if g is None else dev(ctx, g)
                    out = plan._edge_sum(dev(ctx, w), gd, 0.2, transposed)
                    again = plan._edge_sum(dev(ctx, w), gd, 0.2, transposed)
                    assert same_bits(out, again)
                    _, mag, exact, d = GR.edge_sum(rp, ad, n_cols, w, gate=g, slope=0.2, transposed=transposed)
                    err, bound = np.abs(host(out).astype(np.float64) - exact), GR.sum_bound(d)[:, None] * mag
                    worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
                    assert np.all(err <= bound), (H, transposed, g is not None, float(err.max()))      # every value: an empty row has bound 0 and must be 0
        plan.close()
    print("largest error / bound", worst)


# ---- the gradients ----
def test_u_add_v_backward_is_the_two_c_sums(ctx, long_csr):
    A = api()
    rowptr, adj, _ = long_csr
    rng = np.random.default_rng(12)
    n, E = len(rowptr) - 1, len(adj)
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    for H, slope in ((4, 0.2), (3, None), (1, 0.0)):
        s, t = rng.standard_normal((n, H)).astype(np.float32), rng.standard_normal((N_COLS, H)).astype(np.float32)
        ge = dev(ctx, rng.standard_normal((E, H)).astype(np.float32))
        st_, tt = dev(ctx, s).requires_grad_(True), dev(ctx, t).requires_grad_(True)
        e = A.u_add_v(plan, st_, tt, slope)
        e.backward(ge)
        gate, c_slope = (None, 1.0) if slope is None else (e.detach(), slope)
        assert same_bits(st_.grad, plan._edge_sum(ge, gate, c_slope, False)) and same_bits(tt.grad, plan._edge_sum(ge, gate, c_slope, True))
        want_s, want_t = GR.score_backward64(rowptr, adj, N_COLS, host(e), host(ge), float(np.float32(1.0 if slope is None else slope)))
        d_s, d_t = np.diff(rowptr), np.bincount(adj, minlength=N_COLS)
        mag = GR.edge_sum(rowptr, adj, N_COLS, host(ge), gate=None if gate is None else host(gate), slope=c_slope)[1]
        assert np.all(np.abs(host(st_.grad) - want_s) <= GR.sum_bound(d_s)[:, None] * mag)
        mag = GR.edge_sum(rowptr, adj, N_COLS, host(ge), gate=None if gate is None else host(gate), slope=c_slope, transposed=True)[1]
        assert np.all(np.abs(host(tt.grad) - want_t) <= GR.sum_bound(d_t)[:, None] * mag)
    plan.close()
    # needs_input_grad: a gradient for s alone runs no transposed sum and builds no transpose; one-dimensional terms get one-dimensional gradients
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    s1, t1 = dev(ctx, s[:, 0]).requires_grad_(True), dev(ctx, t[:, 0])
    A.u_add_v(plan, s1, t1, 0.2).backward(ge[:, 0])
    assert plan.info()["transposed"] == 0 and tuple(s1.grad.shape) == (n,)
    t1.requires_grad_(True)
    A.u_add_v(plan, s1.detach(), t1, 0.2).backward(ge[:, 0])
    assert plan.info()["transposed"] == 1 and tuple(t1.grad.shape) == (N_COLS,)
    # the gradient reaches the leaf behind a column slice
    leaf = torch.zeros((n, 8), device=ctx.device, requires_grad=True)
    A.u_add_v(plan, leaf[:, 4:5], dev(ctx, t[:, :1]), 0.2).backward(ge[:, :1])
    assert bool((leaf.grad[:, :4] == 0).all()) and bool((leaf.grad[:, 5:] == 0).all()) and bool((leaf.grad[:, 4] != 0).any())
    plan.close()


def test_edge_sum_backward_is_the_broadcast(ctx, long_csr):
    A = api()
    rowptr, adj, _ = long_csr
    rng = np.random.default_rng(13)
    n, E = len(rowptr) - 1, len(adj)
    row = GR.row_index(rowptr)
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    for H in (4, 1):
        wv = ints(rng, E, H)
        for transposed, rows, index in ((False, n, row), (True, N_COLS, adj.astype(np.int64))):
            w = dev(ctx, wv).requires_grad_(True)
            g = rng.standard_normal((rows, H)).astype(np.float32)
            out = A.edge_sum(plan, w, transposed=transposed)
            assert np.array_equal(host(out), GR.edge_sum(rowptr, adj, N_COLS, wv, transposed=transposed)[0])
            out.backward(dev(ctx, g))
            broadcast = plan._edge_add(None, dev(ctx, g), H, 1.0) if transposed else plan._edge_add(dev(ctx, g), None, H, 1.0)
            assert same_bits(w.grad, broadcast) and np.array_equal(bits(host(w.grad)), bits(g[index]))
    w1 = dev(ctx, wv[:, 0]).requires_grad_(True)                       # (E,) gives (n_rows,)
    out = A.edge_sum(plan, w1)
    assert tuple(out.shape) == (n,) and np.array_equal(host(out), GR.edge_sum(rowptr, adj, N_COLS, wv[:, 0])[0][:, 0])
    out.sum().backward()
    assert bool((w1.grad == 1).all())
    plan.close()


def torch_gat(rowptr, adj, s, t, v, slope):
    """the whole formulation on torch CPU float64 leaves"""
    n, H = s.shape
    Dv = v.shape[1] // H
    row, a = torch.as_tensor(GR.row_index(rowptr)), torch.as_tensor(adj.astype(np.int64))
    e = torch.nn.functional.leaky_relu(s[row] + t[a], slope)
    w = torch.cat([torch.softmax(e[rowptr[i]:rowptr[i + 1]], 0) for i in range(n)])
    return torch.zeros((n, H, Dv), dtype=torch.float64).index_add_(0, row, w[:, :, None] * v[a].view(-1, H, Dv)).view(n, H * Dv)


def test_gat_attention_exact_with_zero_terms_on_rows_of_power_of_two_length(ctx, monkeypatch):
    """s = t = 0: every score is 0, every weight 1 / len, a power of two; with integer v, g in [-4, 4] every gradient is a sum of dyadic numbers whose
    partial sums are exact in float32 (a multiple of 2^-16 below 2^7), and the gate at 0 takes the slope 0.25 as torch does: out, grad s, grad t and
    grad v equal torch CPU float64 autograd exactly.  Lengths 1 .. 128 under the shrunk bounds: every class, 128: two chunks."""
    A = api()
    shrink(monkeypatch)
    rng = np.random.default_rng(15)
    lengths = [1, 2, 4, 8, 16, 32, 64, 128, 0, 128]
    rowptr, adj = csr_of(lengths, 23, rng)
    n, H, Dv = len(lengths), 2, 3
    v, g = (rng.integers(-4, 5, shape).astype(np.float32) for shape in ((23, H * Dv), (n, H * Dv)))
    plan = plan_of(ctx, rowptr, adj, 23)
    st_, tt, vt = torch.zeros((n, H), device=ctx.device, requires_grad=True), torch.zeros((23, H), device=ctx.device, requires_grad=True), dev(ctx, v).requires_grad_(True)
    out = A.gat_attention(plan, st_, tt, vt, negative_slope=0.25)
    (out * dev(ctx, g)).sum().backward()
    sc, tc, vc = torch.zeros((n, H), dtype=torch.float64, requires_grad=True), torch.zeros((23, H), dtype=torch.float64, requires_grad=True), torch.tensor(v.astype(np.float64), requires_grad=True)
    ref = torch_gat(rowptr, adj, sc, tc, vc, 0.25)
    (ref * torch.as_tensor(g.astype(np.float64))).sum().backward()
    for got, want, what in ((out, ref.detach(), "out"), (st_.grad, sc.grad, "grad s"), (tt.grad, tc.grad, "grad t"), (vt.grad, vc.grad, "grad v")):
        assert np.array_equal(host(got).astype(np.float64), want.numpy()), what
    # (grad s is 0: the entry gradients of a softmax add up to 0 over a row, and every entry of the row has the same gate; grad t mixes rows)
    assert not sc.grad.any() and tc.grad.abs().sum() > 0 and vc.grad.abs().sum() > 0
    plan.close()


def test_gat_attention_is_its_three_parts_and_real_valued_within_the_bounds(ctx, long_csr):
    """gat_attention equals spmm(edge_softmax(u_add_v)) bit for bit, forward and every gradient; out is within the bound composed in
    gat_reference.attention; every backward stage, fed what the device fed it, is within its own derived bound of the float64 restatement"""
    A = api()
    rowptr, adj, _ = long_csr
    rng = np.random.default_rng(14)
    n, E, H, Dv, slope = len(rowptr) - 1, len(adj), 4, 2, 0.2
    plan = plan_of(ctx, rowptr, adj, N_COLS)
    s, t, v = (rng.standard_normal(shape).astype(np.float32) for shape in ((n, H), (N_COLS, H), (N_COLS, H * Dv)))
    g = rng.standard_normal((n, H * Dv)).astype(np.float32)
    gd = dev(ctx, g)
    runs = []
    for whole in (True, False):
        st_, tt, vt = (dev(ctx, x).requires_grad_(True) for x in (s, t, v))
        if whole:
            out, w = A.gat_attention(plan, st_, tt, vt, negative_slope=slope, return_weights=True)
        else:
            w = A.edge_softmax(plan, A.u_add_v(plan, st_, tt, slope))
            out = A.spmm(plan, w, vt)
        out.backward(gd)
        runs.append((out.detach(), w.detach(), st_.grad, tt.grad, vt.grad))
    assert tuple(runs[0][1].shape) == (E, H) and all(same_bits(p, r) for p, r in zip(*runs))
    out, w, gs, gt, gv = runs[0]
    r = GR.attention(rowptr, adj, s, t, v, slope)
    err = np.abs(host(out).astype(np.float64) - r["out"])
    print("out: largest error", float(err.max()), "largest bound", float(r["bound"].max()))
    assert np.all(err <= r["bound"])
    # the backward, stage by stage on the device's own intermediates: the chain autograd ran, bit for bit, and each stage within its bound
    e = plan._edge_add(dev(ctx, s), dev(ctx, t), H, slope)
    gw = plan._sddmm_heads(gd, dev(ctx, v), H)
    ge = plan._edge_softmax_backward_heads(w, gw)
    assert same_bits(gs, plan._edge_sum(ge, e, slope, False)) and same_bits(gt, plan._edge_sum(ge, e, slope, True))
    assert same_bits(gv, plan._backward_heads(gd, 0, w, H))
    _, mag, exact = HR.sddmm(rowptr, adj, g, v, H)
    assert np.all(np.abs(host(gw) - exact) <= ER.dot_bound(Dv) * mag)
    _, exact, mag = HR.edge_softmax_backward(rowptr, host(w), host(gw))
    assert np.all(np.abs(host(ge) - exact) <= ER.softmax_backward_bound(np.diff(rowptr)[GR.row_index(rowptr)])[:, None] * mag)
    for got, transposed in ((gs, False), (gt, True)):
        _, mag, exact, d = GR.edge_sum(rowptr, adj, N_COLS, host(ge), gate=host(e), slope=slope, transposed=transposed)
        assert np.all(np.abs(host(got) - exact) <= GR.sum_bound(d)[:, None] * mag)
    _, mag, exact = HR.run_transposed(rowptr, adj, N_COLS, g, "sum", host(w))
    assert np.all(np.abs(host(gv) - exact) <= AR.tolerance(np.bincount(adj, minlength=N_COLS))[:, None] * mag)
    # the whole backward against float64 autograd of the whole formulation: close (the stages above carry the bounds)
    ref = GR.attention(rowptr, adj, s, t, v, slope, g=g)
    for got, want, what in ((gs, ref["gs"], "grad s"), (gt, ref["gt"], "grad t"), (gv, ref["gv"], "grad v")):
        assert np.allclose(host(got), want, rtol=1e-3, atol=1e-4), what
    # one head: n x 1 terms keep E x 1 weights as graph_attention(heads=1) does, one-dimensional terms have (E,) weights; the same bits
    o1, w1 = A.gat_attention(plan, dev(ctx, s[:, :1]), dev(ctx, t[:, :1]), dev(ctx, v), slope, return_weights=True)
    o0, w0 = A.gat_attention(plan, dev(ctx, s[:, 0]), dev(ctx, t[:, 0]), dev(ctx, v), slope, return_weights=True)
    assert tuple(w1.shape) == (E, 1) and tuple(w0.shape) == (E,) and same_bits(w1[:, 0], w0) and same_bits(o1, o0) and same_bits(w0, w[:, 0])
    plan.close()


def test_sampled_blocks_two_layer_gat_chain_with_four_heads(ctx):
    """sample_blocks on RMAT-10 x 8, two hops, from_block; each layer is a GAT layer with 4 heads: the terms are the head-wise projections of the
    features on two attention vectors (torch), the layer attends from a block's seeds over its sampled entries.  Forward, layer by layer, within the
    bound of gat_reference.attention (the input of a layer is data: the device's own); the gradient of the features through both layers has the
    same bits on a second run."""
    A = api()
    rng = np.random.default_rng(16)
    src, dst = ctx.gen_rmat(10, 8, 5)
    g = A.Graph.from_coo(ctx, 1 << 10, src, dst)
    seeds = torch.tensor(rng.choice(1 << 10, 64, replace=False).astype(np.int32), device=ctx.device)
    blocks = A.sample_blocks(g, seeds, [6, 4], seed=11, direction="in")
    (p0, cols0), (p1, cols1) = A.AggregationPlan.from_block(ctx, blocks[0]), A.AggregationPlan.from_block(ctx, blocks[1])
    F, H = 16, 4
    a_src, a_dst = (dev(ctx, (rng.standard_normal((H, F // H)) * 0.5).astype(np.float32)) for _ in range(2))
    at1, at0 = torch.searchsorted(cols1, blocks[1]["seeds"]).long(), torch.searchsorted(cols0, blocks[0]["seeds"]).long()

    def layer(plan, x, at, keep):
        s, t = (x[at].view(-1, H, F // H) * a_src).sum(-1), (x.view(-1, H, F // H) * a_dst).sum(-1)
        out = A.gat_attention(plan, s, t, x)
        keep.append((plan, s.detach(), t.detach(), x.detach(), out.detach()))
        return out

    grads = []
    for _ in range(2):
        x = dev(ctx, (np.random.default_rng(17).standard_normal((p1.n_cols, F)) * 0.5).astype(np.float32)).requires_grad_(True)
        keep = []
        h1 = layer(p1, x, at1, keep)
        h0 = layer(p0, h1, at0, keep)
        h0.square().sum().backward()
        grads.append(x.grad.clone())
    assert tuple(h1.shape) == (cols0.numel(), F) and tuple(h0.shape) == (64, F)
    assert same_bits(grads[0], grads[1]) and bool(torch.isfinite(grads[0]).all()) and bool((grads[0] != 0).any())
    for (p, s, t, x, got), what in zip(keep, ("layer 1", "layer 0")):
        r = GR.attention(host(p.rowptr), host(p.adj), host(s), host(t), host(x), 0.2)
        err = np.abs(host(got).astype(np.float64) - r["out"])
        print(what, "largest error", float(err.max()), "largest bound", float(r["bound"].max()))
        assert np.all(err <= r["bound"]), what
    p0.close(); p1.close(); g.close()


# ---- refusals, stats, housekeeping ----
def test_c_refusals_come_before_any_write_and_the_stats_term_by_term(ctx):
    A, L = api(), lib()
    lb = ctx.L
    rng = np.random.default_rng(19)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    h = plan.h
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s, t = dev(ctx, ints(rng, 3, 2)), dev(ctx, ints(rng, 4, 2))
    e, w = torch.full((5, 2), 77.0, device=ctx.device), torch.full((5, 2), 77.0, device=ctx.device)
    out, gx = torch.full((3, 2), 77.0, device=ctx.device), torch.full((4, 2), 77.0, device=ctx.device)
    other = A.Context(0)
    add, total = lb.vgl_hip_agg_edge_add_heads, lb.vgl_hip_agg_edge_sum_heads
    nan, inf = float("nan"), float("inf")
    refused = [
        add(None, h, ptr(s), 2, ptr(t), 2, 2, 0.2, ptr(e), None), add(ctx.h, None, ptr(s), 2, ptr(t), 2, 2, 0.2, ptr(e), None),
        add(ctx.h, h, ptr(s), 2, ptr(t), 2, 2, 0.2, None, None), add(ctx.h, h, None, 2, None, 2, 2, 0.2, ptr(e), None),
        add(ctx.h, h, ptr(s), 2, ptr(t), 2, 0, 0.2, ptr(e), None), add(ctx.h, h, ptr(s), 2, ptr(t), 2, -1, 0.2, ptr(e), None),
        add(ctx.h, h, ptr(s), 1, ptr(t), 2, 2, 0.2, ptr(e), None), add(ctx.h, h, ptr(s), 2, ptr(t), 1, 2, 0.2, ptr(e), None),
        add(ctx.h, h, ptr(s), 2, ptr(t), 2, 2, -0.5, ptr(e), None), add(ctx.h, h, ptr(s), 2, ptr(t), 2, 2, nan, ptr(e), None),
        add(ctx.h, h, ptr(s), 2, ptr(t), 2, 2, inf, ptr(e), None), add(ctx.h, h, ptr(e), 2, ptr(t), 2, 2, 0.2, ptr(e), None),
        add(ctx.h, h, ptr(s), 2, ptr(e[1:]), 2, 2, 0.2, ptr(e), None), add(other.h, h, ptr(s), 2, ptr(t), 2, 2, 0.2, ptr(e), None),
    ]
    for tr, res in ((0, out), (1, gx)):
        refused += [
            total(None, h, ptr(w), ptr(e), 0.2, 2, tr, ptr(res), 2, None), total(ctx.h, None, ptr(w), ptr(e), 0.2, 2, tr, ptr(res), 2, None),
            total(ctx.h, h, None, ptr(e), 0.2, 2, tr, ptr(res), 2, None), total(ctx.h, h, ptr(w), ptr(e), 0.2, 2, tr, None, 2, None),
            total(ctx.h, h, ptr(w), ptr(e), 0.2, 0, tr, ptr(res), 2, None), total(ctx.h, h, ptr(w), ptr(e), 0.2, -3, tr, ptr(res), 2, None),
            total(ctx.h, h, ptr(w), ptr(e), 0.2, 2, tr, ptr(res), 1, None), total(ctx.h, h, ptr(w), ptr(e), -1.0, 2, tr, ptr(res), 2, None),
            total(ctx.h, h, ptr(w), ptr(e), nan, 2, tr, ptr(res), 2, None), total(ctx.h, h, ptr(w), ptr(e), inf, 2, tr, ptr(res), 2, None),
            total(ctx.h, h, ptr(w), ptr(e), 0.2, 2, tr + 2, ptr(res), 2, None), total(ctx.h, h, ptr(w), ptr(e), 0.2, 2, -1, ptr(res), 2, None),
            total(ctx.h, h, ptr(res), ptr(e), 0.2, 2, tr, ptr(res), 2, None), total(ctx.h, h, ptr(w), ptr(res[1:]), 0.2, 2, tr, ptr(res), 2, None),
            total(other.h, h, ptr(w), ptr(e), 0.2, 2, tr, ptr(res), 2, None),
        ]
    assert all(rc != 0 for rc in refused), refused
    assert b"another context" in lb.vgl_hip_last_error()
    ctx.sync()
    assert all(bool((x == 77.0).all()) for x in (e, w, out, gx))
    assert plan.info()["transposed"] == 0                               # a refused transposed sum builds nothing
    # the models, term by term: 5 entries, 3 rows (4 columns), H = 2; three short rows (four) in the list
    st = L.AggStats()
    assert add(ctx.h, h, ptr(s), 2, ptr(t), 2, 2, 0.25, ptr(e), C.byref(st)) == 0
    assert (st.rows, st.entries, st.rows_short, st.vec, st.transposed, st.heads, list(st.column_tiles)) == (3, 5, 3, 1, 0, 2, [1, 1, 1])
    assert st.algorithmic_bytes == 5 * (4 + 4 * 2 + 4 * 2) + 3 * (8 + 4 * 2) + 3 * 4
    assert np.array_equal(bits(host(e)), bits(GR.score(rowptr, adj, host(s), host(t), 0.25)))
    assert add(ctx.h, h, None, 0, ptr(t), 2, 2, 0.25, ptr(w), C.byref(st)) == 0 and st.algorithmic_bytes == 5 * (4 + 4 * 2 + 4 * 2) + 3 * 8 + 3 * 4
    assert add(ctx.h, h, ptr(s), 2, None, 0, 2, 0.25, ptr(w), C.byref(st)) == 0 and st.algorithmic_bytes == 5 * (4 + 4 * 2) + 3 * (8 + 4 * 2) + 3 * 4
    assert add(ctx.h, h, ptr(s), 2, ptr(t), 2, 2, 0.25, ptr(w), None) == 0 and same_bits(w, e)                      # stats may be NULL
    assert total(ctx.h, h, ptr(w), None, 0.25, 2, 0, ptr(out), 2, C.byref(st)) == 0
    assert (st.rows, st.entries, st.vec, st.transposed, st.heads) == (3, 5, 1, 0, 2) and st.algorithmic_bytes == 5 * 4 * 2 + 3 * (8 + 4 * 2) + 3 * 4
    assert total(ctx.h, h, ptr(w), ptr(e), 0.25, 2, 0, ptr(out), 2, C.byref(st)) == 0 and st.algorithmic_bytes == 5 * (4 * 2 + 4 * 2) + 3 * (8 + 4 * 2) + 3 * 4
    assert np.array_equal(host(out), GR.edge_sum(rowptr, adj, 4, host(w), gate=host(e), slope=0.25)[0])
    assert total(ctx.h, h, ptr(w), ptr(e), 0.25, 2, 1, ptr(gx), 2, C.byref(st)) == 0
    assert (st.rows, st.entries, st.rows_short, st.transposed, st.heads) == (4, 5, 4, 1, 2) and st.algorithmic_bytes == 5 * (4 * 2 + 4 * 2 + 4) + 4 * (8 + 4 * 2) + 4 * 4
    assert np.array_equal(host(gx), GR.edge_sum(rowptr, adj, 4, host(w), gate=host(e), slope=0.25, transposed=True)[0])
    assert total(ctx.h, h, ptr(w), None, 0.25, 2, 1, ptr(gx), 2, None) == 0 and plan.info()["transposed"] == 1 and plan.info()["heads"] == 0
    # a leading dimension above H: the columns beside the result stay
    big = torch.full((3, 5), 77.0, device=ctx.device)
    assert total(ctx.h, h, ptr(w), None, 0.25, 2, 0, ptr(big[:, 1:]), 5, None) == 0
    assert bool((big[:, 0] == 77.0).all()) and bool((big[:, 3:] == 77.0).all()) and torch.equal(big[:, 1:3], dev(ctx, GR.edge_sum(rowptr, adj, 4, host(w))[0]))
    other.close()
    plan.close()


def test_python_refusals(ctx):
    A, L = api(), lib()
    rng = np.random.default_rng(18)
    rowptr, adj = csr_of([2, 0, 3], 4, rng)
    plan = plan_of(ctx, rowptr, adj, 4)
    s, t, w, v = dev(ctx, ints(rng, 3, 2)), dev(ctx, ints(rng, 4, 2)), dev(ctx, ints(rng, 5, 2)), dev(ctx, ints(rng, 4, 4))
    for bad, match in ((lambda: A.u_add_v(plan, s.double(), t), "s must be a float32"), (lambda: A.u_add_v(plan, s, t.int()), "t must be a float32"),
                       (lambda: A.u_add_v(plan, s[:2], t), "s must be"), (lambda: A.u_add_v(plan, s, t[:3]), "t must be"),
                       (lambda: A.u_add_v(plan, s, t[:, :1]), "same number of heads"), (lambda: A.u_add_v(plan, s[:, 0], t), "both be one-dimensional"),
                       (lambda: A.u_add_v(plan, s.cpu(), t), "s must live"), (lambda: A.u_add_v(plan, s[:, :, None], t), "s must be"),
                       (lambda: A.u_add_v(plan, s, t, -0.1), "negative_slope"), (lambda: A.u_add_v(plan, s, t, float("nan")), "negative_slope"),
                       (lambda: A.u_add_v(plan, s, t, float("inf")), "negative_slope"), (lambda: A.u_add_v(plan, s, t, "0.2"), "negative_slope"),
                       (lambda: A.u_add_v(plan, s, t, True), "negative_slope"),
                       (lambda: A.edge_sum(plan, w.double()), "w must be a float32"), (lambda: A.edge_sum(plan, w[:4]), "w must hold"),
                       (lambda: A.edge_sum(plan, w.cpu()), "w must hold"), (lambda: A.edge_sum(plan, w, transposed=2), "transposed must be"),
                       (lambda: A.edge_sum(plan, w[:, :0]), "w must hold"),
                       (lambda: A.gat_attention(plan, s, t, v[:, :3]), "of v must be divisible"), (lambda: A.gat_attention(plan, s, t, v[:3]), "v must be n_cols"),
                       (lambda: A.gat_attention(plan, s, t[:, :1], v), "same number of heads"), (lambda: A.gat_attention(plan, s, t, v, -1.0), "negative_slope")):
        with pytest.raises(L.VglHipError, match=match):
            bad()
    plan.close()
    for bad in (lambda: A.u_add_v(plan, s, t), lambda: A.edge_sum(plan, w), lambda: A.gat_attention(plan, s, t, v)):
        with pytest.raises(L.VglHipError, match="open AggregationPlan"):
            bad()


def test_empty_shapes(ctx):
    """no entries, no rows, no heads: empty or zero tensors of the right shape, and gradients of the right shape"""
    A = api()
    plan = plan_of(ctx, np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), 2)
    s, t = torch.ones((3, 2), device=ctx.device, requires_grad=True), torch.ones((2, 2), device=ctx.device, requires_grad=True)
    e = A.u_add_v(plan, s, t, 0.2)
    assert tuple(e.shape) == (0, 2) and A.edge_sum(plan, e).tolist() == [[0.0, 0.0]] * 3 and A.edge_sum(plan, e, transposed=True).tolist() == [[0.0, 0.0]] * 2
    out = A.gat_attention(plan, s, t, torch.ones((2, 4), device=ctx.device))
    assert out.tolist() == [[0.0] * 4] * 3
    out.sum().backward()
    assert s.grad.tolist() == [[0.0, 0.0]] * 3 and t.grad.tolist() == [[0.0, 0.0]] * 2
    assert tuple(A.u_add_v(plan, torch.ones(3, device=ctx.device), torch.ones(2, device=ctx.device)).shape) == (0,)
    plan.close()
    plan = plan_of(ctx, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 2)
    assert tuple(A.gat_attention(plan, torch.ones((0, 2), device=ctx.device), torch.ones((2, 2), device=ctx.device), torch.ones((2, 4), device=ctx.device)).shape) == (0, 4)
    assert tuple(A.edge_sum(plan, torch.ones((0, 2), device=ctx.device)).shape) == (0, 2)
    plan.close()
    rowptr, adj = csr_of([2, 0, 3], 4, np.random.default_rng(20))
    plan = plan_of(ctx, rowptr, adj, 4)
    assert tuple(A.u_add_v(plan, torch.ones((3, 0), device=ctx.device), torch.ones((4, 0), device=ctx.device)).shape) == (5, 0)
    plan.close()


def test_plan_run_destroy_three_times(ctx, long_csr):
    A = api()
    rowptr, adj, _ = long_csr
    rng = np.random.default_rng(17)
    s, t, v = (rng.standard_normal(shape).astype(np.float32) for shape in ((len(LONG), 4), (N_COLS, 4), (N_COLS, 8)))
    seen = []
    for _ in range(3):
        plan = plan_of(ctx, rowptr, adj, N_COLS)
        st_, tt = dev(ctx, s).requires_grad_(True), dev(ctx, t).requires_grad_(True)
        out, w = A.gat_attention(plan, st_, tt, dev(ctx, v), return_weights=True)
        out.sum().backward()
        seen.append((out.detach().clone(), w.detach().clone(), st_.grad.clone(), tt.grad.clone()))
        plan.close()
        assert plan.h is None
    for other in seen[1:]:
        assert all(same_bits(a, b) for a, b in zip(seen[0], other))


@pytest.mark.parametrize("extra", [[], ["-backward"]])
def test_app_check_with_the_additive_score_and_four_heads(extra):
    cmd = [os.path.join(ROOT, "apps", "bin", "attn_hip"), "-gen", "-s", "12", "-e", "16", "-fused", "-score", "add", "-heads", "4", "-check"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "error count: 0" in out.stdout and "heads 4" in out.stdout and "ATTN score (add)" in out.stdout, out.stdout
    assert ("grad s" in out.stdout) == bool(extra)
    bad = subprocess.run(cmd[:-1 - len(extra)] + ["-slope", "-1"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "-slope" in bad.stdout
