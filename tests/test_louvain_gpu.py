"""Louvain move rounds on the GPU (vgl_hip_louvain_move, api.louvain_move) against the restatement of the contract (tests/louvain_reference.py)
on the stored CSR as it is.  Every output is an integer and a function of the graph in its own numbering, the weights and the
arguments: plain equality, the statistics included."""
import ctypes as C

import numpy as np
import pytest
import torch

import louvain_reference as R
import quotient_reference as QR

pytestmark = pytest.mark.gpu
SWITCHES = ("VGL_LOUVAIN_SHORT", "VGL_LOUVAIN_WAVE", "VGL_LOUVAIN_WG", "VGL_LOUVAIN_SORT_CAP_MB")
FOLLOW_SWITCHES = ("rows_short", "rows_wave", "rows_wg", "rows_sorted", "sorted_keys", "sort_pieces")


def api():
    from vectorgraphlibrary_amd import api as A
    return A


def lib():
    from vectorgraphlibrary_amd import lib as L
    return L


def dev(ctx, a, dtype):
    return torch.tensor(np.asarray(a, dtype=dtype), device=ctx.device)


def graph(ctx, V, src, dst, renumber=None):
    return api().Graph.from_coo(ctx, V, dev(ctx, src, np.int32), dev(ctx, dst, np.int32), with_incoming=False, renumber=renumber)


def host(g):
    return g.out_rowptr.cpu().numpy(), g.out_adj.cpu().numpy()


def set_switches(monkeypatch, short=None, wave=None, wg=None, cap_mb=None):
    for name, val in zip(SWITCHES, (short, wave, wg, cap_mb)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    d = lambda v, dflt: dflt if v is None else v
    return {"short": d(short, R.SHORT), "wave": d(wave, R.WAVE), "wg": d(wg, R.WG), "cap_mb": d(cap_mb, R.CAP_MB)}


def own_simple(g, weights=None):
    """the restatement's level-0 graph from the handle's own stored CSR"""
    rowptr, adj = host(g)
    return R.simple_graph(g.V, QR.rows_of(rowptr), adj, weights)


def check_move(ctx, V, rowptr, adj, w=None, what="", **kw):
    """api.louvain_move on the stored CSR (rowptr, adj) as it is, against the restatement"""
    A = api()
    g = A.Graph(ctx, V, dev(ctx, rowptr, np.int64), dev(ctx, adj, np.int32))
    labels, info = A.louvain_move(g, None if w is None else torch.tensor(w), raw=True, **kw)
    ref_labels, ref = R.move(rowptr, adj, w, kw.get("max_rounds", 64), kw.get("min_gain_den", 0), kw.get("seed", 0))
    print("louvain_move", what, {k: info[k] for k in ("rounds", "communities", "outcome", "modularity_num")})
    assert labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), ref_labels), what
    got = (info["levels"], info["total_weight"], info["modularity_num"], info["rounds"], info["outcome"], info["communities"], info["vertices"], info["entries"])
    assert got == (1, ref["m"], ref["N"], [ref["rounds"]], [ref["outcome"]], [ref["communities"]], [V], [len(adj)]), (what, got, ref)
    g.close()
    return labels, info


def rmat(ctx, scale, ef, seed):
    src, dst = (t.cpu().numpy() for t in ctx.gen_rmat(scale, ef, seed))
    return 1 << scale, src, dst


def simple_of(ctx, name):
    V, src, dst = rmat(ctx, 10, 8, 5) if name == "rmat10" else rmat(ctx, 12, 16, 1) if name == "rmat12" else R.fixed_graphs()[name]
    rowptr, adj, _ = R.simple_graph(V, src, dst)
    return V, rowptr, adj


# ---- 1. the fixed graphs and RMAT-10x8: the level on the simple graph, and on its coarse graph (self entries, weights) ----
def test_fixed_graphs_and_rmat(ctx, monkeypatch):
    set_switches(monkeypatch)
    seen = set()
    for name in list(R.fixed_graphs()) + ["rmat10"]:
        V, rowptr, adj = simple_of(ctx, name)
        for seed in (0, 1):
            labels, info = check_move(ctx, V, rowptr, adj, None, what="%s / seed %d" % (name, seed), seed=seed)
            seen |= set(info["outcome"])
            if info["communities"][0] < V:
                q_rowptr, q_adj, q_count = QR.quotient_dir(rowptr, adj, labels.cpu().numpy(), None, False)
                _, info = check_move(ctx, len(q_rowptr) - 1, q_rowptr, q_adj, q_count, what="%s / seed %d / coarse" % (name, seed), seed=seed + (1 << 16))
                seen |= set(info["outcome"])
    assert "converged" in seen and "reverted" in seen, seen


def test_original_order_translates_the_labels(ctx, monkeypatch):
    set_switches(monkeypatch)
    A = api()
    V, src, dst = rmat(ctx, 10, 8, 5)
    both = (np.concatenate([src, dst]), np.concatenate([dst, src]))
    g = graph(ctx, V, both[0], both[1], "total")
    own, _ = A.louvain_move(g, raw=True)
    orig, _ = A.louvain_move(g)
    assert g.fwd is not None and torch.equal(orig, g.to_original(g.bwd[own.long()].to(torch.int32).contiguous()))
    rowptr, adj = host(g)
    ref, _ = R.move(rowptr, adj)
    assert np.array_equal(own.cpu().numpy(), ref)
    # the partition is the own one: two vertices share a label in ORIGINAL order iff their own images do
    o = orig.cpu().numpy()
    f = g.fwd.cpu().numpy()
    assert np.array_equal(o[:, None] == o[None, :], (ref[f][:, None] == ref[f][None, :]))


# ---- 2. classes and bounds ----
@pytest.mark.parametrize("L", [32, 33, 1024, 1025, 4096, 4097])
def test_class_bounds_under_the_defaults(ctx, monkeypatch, L):
    set_switches(monkeypatch)
    V, src, dst = (L + 1,) + QR._both([(0, i) for i in range(1, L + 1)])
    rowptr, adj, _ = QR.coo_to_csr(V, src, dst)
    labels, info = check_move(ctx, V, rowptr, adj, None, what="star %d" % L)
    cls = "rows_short" if L <= 32 else "rows_wave" if L <= 1024 else "rows_wg" if L <= 4096 else "rows_sorted"
    assert info[cls] == (L + 1 if L <= 32 else 1)
    assert info["sort_pieces"] == (1 if L > 4096 else 0)
    pairs = [(0, 1)] + [(0, 2 + i) for i in range(L - 1)] + [(1, 1 + L + i) for i in range(L - 1)]
    V, src, dst = (2 * L,) + QR._both(pairs)
    rowptr, adj, _ = QR.coo_to_csr(V, src, dst)
    _, info = check_move(ctx, V, rowptr, adj, None, what="double star %d" % L)
    assert info[cls] >= 2


@pytest.mark.parametrize("name", ["rmat10", "rmat12"])
def test_every_class_with_small_bounds(ctx, monkeypatch, name):
    """a 1 MB cap holds 32768 keys: RMAT-12x16 has more in its sorted rows, so its pieces are cut"""
    V, rowptr, adj = simple_of(ctx, name)
    w = np.random.default_rng(4).integers(0, 9, size=len(adj) // 2).astype(np.int64)
    rows = QR.rows_of(rowptr)
    order = np.lexsort((np.maximum(rows, adj), np.minimum(rows, adj)))        # the two slots of an edge are neighbours in this order
    sw = np.empty(len(adj), dtype=np.int64)
    sw[order] = np.repeat(w, 2)
    for wt in (None, sw):
        set_switches(monkeypatch)
        l0, i0 = check_move(ctx, V, rowptr, adj, wt, what=name + " defaults")
        set_switches(monkeypatch, 4, 16, 64, 1)
        l1, i1 = check_move(ctx, V, rowptr, adj, wt, what=name + " small bounds, cap 1 MB")
        set_switches(monkeypatch)
        assert torch.equal(l0, l1)
        assert all(i1[k] > 0 for k in FOLLOW_SWITCHES), i1
        assert i1["sort_pieces"] >= (2 if name == "rmat12" else 1)
        assert {k: v for k, v in i0.items() if k not in FOLLOW_SWITCHES} == {k: v for k, v in i1.items() if k not in FOLLOW_SWITCHES}


# ---- 3. one level on a stored multigraph ----
def test_move_on_stored_multigraphs(ctx, monkeypatch):
    set_switches(monkeypatch)
    rng = np.random.default_rng(11)
    for trial in range(6):                                            # loops, repeats and weight-0 entries
        V = int(rng.integers(2, 200))
        E = int(rng.integers(1, 6 * V))
        s, d = rng.integers(0, V, size=E), rng.integers(0, V, size=E)
        rowptr, adj, perm = QR.coo_to_csr(V, np.concatenate([s, d]), np.concatenate([d, s]))
        ew = rng.integers(0, 6, size=E)
        w = np.concatenate([ew, ew])[perm].astype(np.int64)
        check_move(ctx, V, rowptr, adj, None, what="multigraph %d" % trial, seed=trial)
        check_move(ctx, V, rowptr, adj, w, what="multigraph %d weighted" % trial, seed=trial)
    # a row whose entries all fall into one community: 40 (then 1500, 5000) copies of one edge next to a triangle
    for copies in (3, 40, 1500, 5000):
        s = [0] * copies + [2, 3, 4]
        d = [1] * copies + [3, 4, 2]
        rowptr, adj, _ = QR.coo_to_csr(5, np.array(s + d), np.array(d + s))
        check_move(ctx, 5, rowptr, adj, None, what="%d copies" % copies)
    # a row all of whose entries are distinct, at the LDS bounds and one past them
    for L in (1024, 4096, 4097):
        V, src, dst = (L + 1,) + QR._both([(0, i) for i in range(1, L + 1)] + [(i, i + 1) for i in range(1, L, 2)])
        rowptr, adj, _ = QR.coo_to_csr(V, src, dst)
        check_move(ctx, V, rowptr, adj, None, what="distinct %d" % L)
    # the coarse graph of ring_of_cliques: self entries that carry the internal weight
    V, src, dst = R.fixed_graphs()["ring_of_cliques"]
    rowptr, adj, _ = R.simple_graph(V, src, dst)
    labels, _ = R.move(rowptr, adj)
    q_rowptr, q_adj, q_count = QR.quotient_dir(rowptr, adj, labels, None, False)
    assert (q_adj == QR.rows_of(q_rowptr)).any()
    check_move(ctx, len(q_rowptr) - 1, q_rowptr, q_adj, q_count, what="coarse ring of cliques", seed=1 << 16)


# ---- 4. the other outcomes, determinism ----
def test_capped_small_gain_and_determinism(ctx, monkeypatch):
    set_switches(monkeypatch)
    V, rowptr, adj = simple_of(ctx, "rmat10")
    _, info = check_move(ctx, V, rowptr, adj, None, what="rmat10 capped", max_rounds=5)
    assert info["outcome"] == ["capped"]
    for name in ("grid12", "gnp300"):                                 # the restatement ends these with a small gain at D = 200
        Vs, rp, ad = simple_of(ctx, name)
        _, info = check_move(ctx, Vs, rp, ad, None, what=name + " small gain", min_gain_den=200)
        assert info["outcome"] == ["small_gain"]
    a, ia = check_move(ctx, V, rowptr, adj, None, what="rmat10")
    b, ib = check_move(ctx, V, rowptr, adj, None, what="rmat10 again")
    assert torch.equal(a, b) and ia == ib


# ---- 5. refusals ----
def test_failures_leave_the_outputs_untouched(ctx):
    A, L = api(), lib()
    V, src, dst = R.fixed_graphs()["caveman"]
    g = graph(ctx, V, src, dst)
    fill = -7
    label = torch.full((V,), fill, dtype=torch.int32, device=ctx.device)
    st = L.LouvainStats()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ok_w = torch.ones(g.E, dtype=torch.int64, device=ctx.device)
    neg_w = ok_w.clone()
    neg_w[3] = -1
    big_w = torch.full((g.E,), (1 << 31) // g.E + 1, dtype=torch.int64, device=ctx.device)
    huge_w = ok_w.clone()
    huge_w[0] = (1 << 62)

    def move(ctx_h=ctx.h, g_h=g.h, w=None, max_rounds=64, D=0, out=label):
        return ctx.L.vgl_hip_louvain_move(ctx_h, g_h, p(w), max_rounds, D, 0, p(out), C.byref(st))

    shard = g.shard(0, V // 2)
    bad = [dict(ctx_h=None), dict(g_h=None), dict(out=None), dict(g_h=shard.h), dict(max_rounds=0), dict(max_rounds=65536), dict(D=-1), dict(w=neg_w),
           dict(w=big_w), dict(w=huge_w)]
    for kw in bad:
        assert move(**kw) != 0, kw
    ctx.sync()
    assert bool((label == fill).all())
    with pytest.raises(L.VglHipError):
        A.louvain_move(g, max_rounds=0)
    with pytest.raises(L.VglHipError):
        A.louvain_move(g, weights=neg_w)
    with pytest.raises(L.VglHipError):
        A.louvain_move(g, weights=big_w)
    assert move() == 0
